// Tile pre-processing on the device: the reference finalises every cached uint8 ROI on the host
// with torchvision/Pillow (RoiBuilder.py:193-210: Pad(100) -> RandomCrop(roi) -> Resize(res) -> flips -> ToTensor ->
// Normalize(0.5, 0.5)) and then uploads fp32 tiles.  Here the cached uint8 ROIs stay resident in HBM (2500 x 4.3 MB
// per slide fits easily in 288 GB) and one kernel produces the fp32 NCHW tile stack the encoder reads.
//
// Arithmetic = Pillow's two-pass bilinear resampling, restated (not linked): per output sample a support-scaled
// triangle filter, normalised in float64 and rounded to 22-bit fixed point (host: mil_resize_coeffs), horizontal
// pass to uint8, vertical pass to uint8, each with a half-ulp bias and saturation — bit-exact against Pillow
// (tests/golden/prep_*.npz).  Padding and cropping are index arithmetic: every staged source row sits between two
// zero margins of `pad` pixels in LDS, so taps never need a bounds test; flips are applied at the store.
//
// One workgroup = 8 output rows of one tile: their ~8*scale + 2*support source rows are staged four at a time with
// aligned 4-byte loads, filtered horizontally into an LDS strip [rows][res][3], then the strip is filtered vertically.
//
// Windows of a slide (WIN = true, mil_tile_preprocess_win*): the ROI is not a tile of a contiguous stack but a window of a
// larger image that stays where it is — row y of window t starts at byte win_off[t] + y * row_pitch of the source, at ANY byte
// alignment, and the phase (win_off + y * pitch) & 15 changes from row to row whenever the pitch is no multiple of 16.  A
// row is staged as the 16-byte granules of the SOURCE's own grid that hold its bytes, each fetched with one aligned load
// and stored, unshifted, at the same granule of the LDS row: the row's first byte then sits at margin + phase instead of
// margin, and the horizontal pass — which funnel-shifts its taps to the window start anyway — adds the row's phase to the
// shift.  Masking: left and right of a window the slide has real pixels, and Pad() pads with zeros; every granule is ANDed
// with the mask of its bytes that belong to the row (all ones except in the first and the last granules), so the bytes in
// front of and behind a staged row are zero in LDS exactly as they are for a stack, and rows of the padded image outside
// the window are stored as zeros whatever the source holds there.  Bounds: every load goes through a buffer descriptor from
// the grid point below the workgroup's first row to the end of the source rounded up to the grid (roi_select.hip), so an
// over-fetch in front of the first or behind the last window returns zeros; its 32-bit offsets are relative to that row
// (host: rows of a band * pitch < 2 GiB) while win_off and y * pitch are 64-bit.  A source whose rows all start on the
// grid — a contiguous stack with 3S % 16 == 0, a slide with base, 3W and 3 * col multiples of 16 — needs no extra granule
// per row and stages exactly the pieces the stack kernel's fast path does.
#include "pf_common.cuh"
#include <cmath>

#define PREP_BITS 22
#define PREP_BAND 8
#define PREP_ROWS 4

struct PrepArgs {
    const uint8_t* rois;        // [T,S,S,3]
    const int* params;          // [T,4] = top, left, hflip, vflip (train chain) or null (flat chain: no pad/crop/flip)
    const int* bounds;          // [R,2] first source index, count
    const int* kk;              // [R,ksize]
    float* out;                 // [T,3,R,R] fp32 NCHW, or null when xs is given
    __bf16* xs;                 // [T,R/2,R/2,16] bf16 space-to-depth NHWC (channel = c*4 + dy*2 + dx, 12 real), or null
    uint8_t* out_u8;            // [T,3,R,R] the resized bytes themselves, planar (the uint8 feed: u8_feed.cuh), or null
    int T, S, pad, R, ksize;
    int margin, row_pitch;      // bytes: zero margin in front of a staged row (>= 3*pad, 4-aligned); pitch of a staged row
    int lds_h_off, lds_k_off, lds_b_off;
    // WIN only: the source as mil_roi_stats takes it
    const uint8_t* base_al;     // source pointer rounded down to the 16-byte grid
    const long long* win_off;   // [T] byte offset of each window's first pixel from the (unrounded) source pointer
    long long total;            // bytes from base_al to the grid point at or behind the end of the source
    long long src_pitch;        // bytes between two rows of a window
    int delta;                  // source pointer - base_al (0..15)
};

__device__ __forceinline__ unsigned prep_clip8(int v) { v >>= PREP_BITS; return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// all ones in the bytes b of a dword with lo <= b < hi (byte 0 = the lowest address), zero elsewhere
__device__ __forceinline__ unsigned prep_keep(int lo, int hi) {
    lo = min(max(lo, 0), 4); hi = min(max(hi, 0), 4);
    const unsigned mh = hi == 4 ? ~0u : (1u << (8 * hi)) - 1u, ml = lo == 4 ? ~0u : (1u << (8 * lo)) - 1u;
    return mh & ~ml;
}

template <int KS, bool WIN>
__global__ __launch_bounds__(256) void tile_preprocess_kernel(PrepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    MIL_POISON(psm);
    unsigned char* rows = psm;
    unsigned char* hres = psm + a.lds_h_off;
    int* kks = reinterpret_cast<int*>(psm + a.lds_k_off);
    int* bds = reinterpret_cast<int*>(psm + a.lds_b_off);
    const int tid = threadIdx.x, t = blockIdx.y;
    const int S = a.S, R = a.R, ksize = a.ksize;
    for (int i = tid; i < R * ksize; i += 256) kks[i] = a.kk[i];
    for (int i = tid; i < 2 * R; i += 256) bds[i] = a.bounds[i];
    for (int i = tid * 4; i < PREP_ROWS * a.row_pitch; i += 1024) *reinterpret_cast<unsigned*>(rows + i) = 0u;   // margins stay zero
    int top = 0, left = 0, hflip = 0, vflip = 0, pad = 0;
    if (a.params) { top = a.params[4 * t]; left = a.params[4 * t + 1]; hflip = a.params[4 * t + 2]; vflip = a.params[4 * t + 3]; pad = a.pad; }
    __syncthreads();
    const int r0 = blockIdx.x * PREP_BAND, r1 = min(r0 + PREP_BAND, R);
    const int y_lo = bds[2 * r0], y_hi = bds[2 * (r1 - 1)] + bds[2 * (r1 - 1) + 1];
    const int nri = y_hi - y_lo;
    const unsigned char* src_tile = WIN ? nullptr : a.rois + (size_t)t * S * S * 3;
    const int row_bytes = S * 3;
    const bool wide = !WIN && (row_bytes & 3) == 0 && (reinterpret_cast<uintptr_t>(src_tile) & 3) == 0;

    // WIN: descriptor of this workgroup, from the grid point below the first source row it reads to the end of the source
    // (no row: range 0).  rel0 = that row's first byte inside the descriptor; phase of source row ys = (rel0 + (ys - ys0) * pitch) & 15.
    const long long woff = WIN ? a.win_off[t] : 0;
    const int ys0 = WIN ? max(top + y_lo - pad, 0) : 0;
    const long long fb = (long long)a.delta + woff + (long long)ys0 * a.src_pitch;
    const long long B = fb & ~15ll, room = a.total - B;
    const unsigned range = (!WIN || woff < 0 || ys0 >= S || room <= 0) ? 0u : (room > 0x80000000ll ? 0x80000000u : (unsigned)room);
    const __amdgpu_buffer_rsrc_t rs = mil_rsrc(WIN ? a.base_al + B : nullptr, range);
    const unsigned rel0 = (unsigned)(fb - B), spitch = (unsigned)a.src_pitch;
    const bool grid_rows = (fb & 15) == 0 && (a.src_pitch & 15) == 0;         // every row of the window starts on the 16-byte grid

    // Fast path (16-byte aligned rows, <= 4 KB each): the next four source rows are fetched into registers while the
    // current four are filtered, so the global-load latency is paid once per band instead of once per row group.
    typedef __attribute__((ext_vector_type(4))) unsigned u4_t;
    // (WIN: granules of the source grid per row — one more than the row's own when rows may start anywhere in a granule)
    const int ppr = WIN ? (row_bytes + (grid_rows ? 15 : 30)) >> 4 : row_bytes >> 4;      // 16-byte pieces per source row
    const bool fast = WIN ? ppr <= 256
                          : (row_bytes & 15) == 0 && (a.margin & 15) == 0 && (reinterpret_cast<uintptr_t>(src_tile) & 15) == 0 && ppr <= 256;
    // WIN: granule `piece` of row j of the band (row ys of the window), masked to the bytes that are the row's
    auto win_piece = [&](int j, int piece) -> u4_t {
        const int ys = top + y_lo + j - pad;
        const bool ok = j < nri && ys >= 0 && ys < S;
        const unsigned r = rel0 + (unsigned)(ys - ys0) * spitch;
        const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? (r & ~15u) + 16u * (unsigned)piece : MIL_OOB, 0, 0);
        const int lo = ok ? (int)(r & 15u) - 16 * piece : 0, hi = ok ? lo + row_bytes : 0;
        u4_t v = q;
        if (lo > 0 || hi < 16) {                                      // a row's first and last granules only (and rows that are not there)
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] = q[d] & prep_keep(lo - 4 * d, hi - 4 * d);
        }
        return v;
    };
    u4_t pre[PREP_ROWS];
    auto fetch_rows = [&](int j0) {
#pragma unroll
        for (int i = 0; i < PREP_ROWS; ++i) {
            const int id = tid + 256 * i, jj = id / ppr, piece = id - jj * ppr;
            if constexpr (WIN) {
                pre[i] = win_piece(jj < PREP_ROWS ? j0 + jj : nri, piece);
            } else {
                const int ys = top + y_lo + j0 + jj - pad;
                const bool ok = jj < PREP_ROWS && j0 + jj < nri && ys >= 0 && ys < S;
                pre[i] = ok ? *reinterpret_cast<const u4_t*>(src_tile + (size_t)ys * row_bytes + piece * 16) : u4_t{0u, 0u, 0u, 0u};
            }
        }
    };
    if (fast) fetch_rows(0);

    for (int j0 = 0; j0 < nri; j0 += PREP_ROWS) {
        // ---- stage up to four source rows (rows of the padded/cropped image; outside the ROI they are zero) ----
        if (fast) {
#pragma unroll
            for (int i = 0; i < PREP_ROWS; ++i) {
                const int id = tid + 256 * i, jj = id / ppr, piece = id - jj * ppr;
                if (jj < PREP_ROWS) *reinterpret_cast<u4_t*>(rows + jj * a.row_pitch + a.margin + piece * 16) = pre[i];
            }
            __syncthreads();
            if (j0 + PREP_ROWS < nri) fetch_rows(j0 + PREP_ROWS);
        } else if constexpr (WIN) {                                   // rows of more than 4 KB: granule by granule, no prefetch
            for (int id = tid; id < PREP_ROWS * ppr; id += 256) {
                const int jj = id / ppr, piece = id - jj * ppr;
                *reinterpret_cast<u4_t*>(rows + jj * a.row_pitch + a.margin + piece * 16) = win_piece(j0 + jj, piece);
            }
            __syncthreads();
        } else {
            for (int jj = 0; jj < PREP_ROWS; ++jj) {
                if (j0 + jj >= nri) break;
                const int ys = top + y_lo + j0 + jj - pad;
                const bool inside = ys >= 0 && ys < S;
                unsigned char* dst = rows + jj * a.row_pitch + a.margin;
                const unsigned char* src = src_tile + (size_t)(inside ? ys : 0) * row_bytes;
                if (wide) {
                    for (int b = tid * 4; b < row_bytes; b += 1024)
                        *reinterpret_cast<unsigned*>(dst + b) = inside ? *reinterpret_cast<const unsigned*>(src + b) : 0u;
                } else {
                    for (int b = tid; b < row_bytes; b += 256) dst[b] = inside ? src[b] : (unsigned char)0;
                }
            }
            __syncthreads();
        }
        // ---- horizontal pass of these rows -> strip ------------------------------------------------------------
        // A thread owns output column xr for all staged rows: its KS weights are read once; the 3*KS source bytes of
        // a row are fetched as aligned dwords and funnel-shifted (v_alignbyte) to the window start, so the taps index
        // registers at compile-time positions (weights beyond the window are zero, the bytes behind them are slack).
        for (int xr = tid; xr < R; xr += 256) {
            constexpr int ND = (3 * KS + 3) / 4;
            const int xmin = bds[2 * xr];
            int w[KS];
#pragma unroll
            for (int k = 0; k < KS; ++k) w[k] = k < ksize ? kks[xr * ksize + k] : 0;
            const int bx = a.margin + (left - pad + xmin) * 3;
            for (int jj = 0; jj < PREP_ROWS; ++jj) {
                if (j0 + jj >= nri) break;
                // WIN: the staged row starts its phase behind the margin (a row outside the window is all zeros: any phase does)
                const int b0 = WIN ? bx + (int)((rel0 + (unsigned)(top + y_lo + j0 + jj - pad - ys0) * spitch) & 15u) : bx;
                const int al = b0 & ~3;
                const unsigned sh = (unsigned)(b0 & 3);
                const unsigned* q = reinterpret_cast<const unsigned*>(rows + jj * a.row_pitch + al);
                unsigned d[ND + 1], e[ND];
#pragma unroll
                for (int i = 0; i < ND + 1; ++i) d[i] = q[i];
#pragma unroll
                for (int i = 0; i < ND; ++i) e[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
                int s0 = 1 << (PREP_BITS - 1), s1 = s0, s2 = s0;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    s0 += (int)((e[(3 * k) >> 2] >> (((3 * k) & 3) * 8)) & 0xffu) * w[k];
                    s1 += (int)((e[(3 * k + 1) >> 2] >> (((3 * k + 1) & 3) * 8)) & 0xffu) * w[k];
                    s2 += (int)((e[(3 * k + 2) >> 2] >> (((3 * k + 2) & 3) * 8)) & 0xffu) * w[k];
                }
                unsigned char* h = hres + ((j0 + jj) * R + xr) * 3;
                h[0] = (unsigned char)prep_clip8(s0); h[1] = (unsigned char)prep_clip8(s1); h[2] = (unsigned char)prep_clip8(s2);
            }
        }
        __syncthreads();
    }
    // ---- vertical pass of the strip, ToTensor + Normalize, flips at the store ---------------------------------------
    if (a.xs) {
        // space-to-depth bf16 output: what the stem kernels consume (the 7x7/s2 conv as a 4x4/s1 conv over 2x2 pixel blocks).
        // A thread owns one 2x2 block of the band = ONE 32-byte record [c0: 00 01 10 11 | c1 .. | c2 .. | 0 0 0 0]; a flip
        // sends a block to the mirrored block and swaps the pixels inside it.  R is even, bands start on even rows.
        const int R2 = R >> 1;
        for (int it = tid; it < ((r1 - r0) >> 1) * R2; it += 256) {
            const int by = it / R2, bx = it - by * R2;
            __bf16 rec[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) rec[j] = (__bf16)0.0f;
            int oby = 0, obx = 0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int yr = r0 + 2 * by + dy, xr = 2 * bx + dx;
                    const int ymin = bds[2 * yr], cnt = bds[2 * yr + 1];
                    const unsigned char* p = hres + ((ymin - y_lo) * R + xr) * 3;
                    const int* w = kks + yr * ksize;
                    int s0 = 1 << (PREP_BITS - 1), s1 = s0, s2 = s0;
                    for (int k = 0; k < cnt; ++k) {
                        const int wk = w[k];
                        s0 += (int)p[k * R * 3] * wk; s1 += (int)p[k * R * 3 + 1] * wk; s2 += (int)p[k * R * 3 + 2] * wk;
                    }
                    const int yo = vflip ? R - 1 - yr : yr, xo = hflip ? R - 1 - xr : xr;
                    oby = yo >> 1; obx = xo >> 1;                       // the same block for all four pixels
                    const int q = (yo & 1) * 2 + (xo & 1);
                    const float v0 = ((float)prep_clip8(s0) / 255.0f - 0.5f) / 0.5f, v1 = ((float)prep_clip8(s1) / 255.0f - 0.5f) / 0.5f,
                                v2 = ((float)prep_clip8(s2) / 255.0f - 0.5f) / 0.5f;
                    // (compile-time register indices: select on q)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        if (q == qq) { rec[qq] = (__bf16)v0; rec[4 + qq] = (__bf16)v1; rec[8 + qq] = (__bf16)v2; }
                    }
                }
            }
            bf16x8_t lo8, hi8;
#pragma unroll
            for (int j = 0; j < 8; ++j) { lo8[j] = rec[j]; hi8[j] = rec[8 + j]; }
            __bf16* o = a.xs + (((size_t)t * R2 + oby) * R2 + obx) * 16;
            *reinterpret_cast<bf16x8_t*>(o) = lo8;
            *reinterpret_cast<bf16x8_t*>(o + 8) = hi8;
        }
        return;
    }
    for (int it = tid; it < (r1 - r0) * R; it += 256) {
        const int yy = it / R, xr = it - yy * R, yr = r0 + yy;
        const int ymin = bds[2 * yr], cnt = bds[2 * yr + 1];
        const unsigned char* p = hres + ((ymin - y_lo) * R + xr) * 3;
        const int* w = kks + yr * ksize;
        int s0 = 1 << (PREP_BITS - 1), s1 = s0, s2 = s0;
        for (int k = 0; k < cnt; ++k) {
            const int wk = w[k];
            s0 += (int)p[k * R * 3] * wk; s1 += (int)p[k * R * 3 + 1] * wk; s2 += (int)p[k * R * 3 + 2] * wk;
        }
        const int yo = vflip ? R - 1 - yr : yr, xo = hflip ? R - 1 - xr : xr;
        const size_t plane = (size_t)R * R;
        if (a.out_u8) {             // Pillow's own bytes: ToTensor + Normalize is left to the stem kernels' decode table
            uint8_t* o8 = a.out_u8 + ((size_t)t * 3 * R + yo) * R + xo;
            o8[0] = (uint8_t)prep_clip8(s0); o8[plane] = (uint8_t)prep_clip8(s1); o8[2 * plane] = (uint8_t)prep_clip8(s2);
            continue;
        }
        float* o = a.out + ((size_t)t * 3 * R + yo) * R + xo;
        o[0] = ((float)prep_clip8(s0) / 255.0f - 0.5f) / 0.5f;
        o[plane] = ((float)prep_clip8(s1) / 255.0f - 0.5f) / 0.5f;
        o[2 * plane] = ((float)prep_clip8(s2) / 255.0f - 0.5f) / 0.5f;
    }
}

// Pillow's coefficient construction for a resize of a whole axis (host, float64 — same operation order as its
// precompute_coeffs / normalize_coeffs_8bpc).  The filter is the triangle (MIL_FILTER_BILINEAR, support 1: what the tile
// chain above resamples with) or the truncated sinc w(x) = sinc(x) sinc(x/3) on [-3, 3) (MIL_FILTER_LANCZOS, support 3: what
// mil_grad_cam resizes its maps with).  Lanczos coefficients can be negative: the half-ulp bias of the fixed-point rounding
// follows the coefficient's sign.
static double prep_filter_support(int filter) { return filter == MIL_FILTER_LANCZOS ? 3.0 : 1.0; }

static double prep_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

static double prep_filter(int filter, double x) {
    if (filter == MIL_FILTER_LANCZOS) return (-3.0 <= x && x < 3.0) ? prep_sinc(x) * prep_sinc(x / 3) : 0.0;
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

static int prep_ksize(int in_size, int out_size, int filter = MIL_FILTER_BILINEAR) {
    double scale = (double)in_size / (double)out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(prep_filter_support(filter) * filterscale) * 2 + 1;
}

static bool prep_filter_ok(int filter) { return filter == MIL_FILTER_BILINEAR || filter == MIL_FILTER_LANCZOS; }

extern "C" int mil_resample_plan(int in_size, int out_size, int filter, int* ksize) {
    if (in_size <= 0 || out_size <= 0 || !prep_filter_ok(filter) || !ksize) return MIL_ERR_ARG;
    *ksize = prep_ksize(in_size, out_size, filter);
    return MIL_OK;
}

extern "C" int mil_resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk) {
    if (in_size <= 0 || out_size <= 0 || !prep_filter_ok(filter) || !bounds || !kk) return MIL_ERR_ARG;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = prep_filter_support(filter) * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / filterscale;
    double* w = new double[ksize];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = prep_filter(filter, (x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        for (int x = 0; x < ksize; ++x) {
            double c = 0.0;
            if (x < xmax) c = (ww != 0.0) ? w[x] / ww : w[x];
            kk[(size_t)xx * ksize + x] = c < 0 ? (int32_t)(-0.5 + c * (double)(1 << PREP_BITS)) : (int32_t)(0.5 + c * (double)(1 << PREP_BITS));
        }
        bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
    }
    delete[] w;
    return MIL_OK;
}

extern "C" int mil_resize_plan(int in_size, int out_size, int* ksize) {
    return mil_resample_plan(in_size, out_size, MIL_FILTER_BILINEAR, ksize);
}

extern "C" int mil_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* kk) {
    return mil_resample_coeffs(in_size, out_size, MIL_FILTER_BILINEAR, bounds, kk);
}

// Windows of a larger source (mil_tile_preprocess_win*): the source convention of mil_roi_stats.
struct PrepWin { const uint8_t* base; int64_t base_bytes; const int64_t* win_off; int64_t row_pitch; };

// out [T,3,R,R] fp32 in [-1,1] from uint8 ROIs [T,S,S,3].  params [T,4] (top, left, hflip, vflip with top/left in
// [0, 2*pad]) selects the train chain, null the flat chain.  bounds_host is the host copy of the table (the launcher
// sizes the LDS strip from it); bounds_dev / kk_dev are its device copies (mil_resize_coeffs(S, R)).  `win` instead of `rois`:
// the ROIs are windows of a larger source (the WIN kernels).
static int prep_entry(const uint8_t* rois, const PrepWin* win, const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                      const int32_t* kk_dev, float* out, void* xs, uint8_t* out_u8, int T, int S, int pad, int R, void* stream) {
    if (win && (!win->base || !win->win_off || win->base_bytes < 0 || S <= 0 || win->row_pitch < 3 * (int64_t)S)) return MIL_ERR_ARG;
    if ((!win && !rois) || !bounds_host || !bounds_dev || !kk_dev || (!out && !xs && !out_u8) || T < 0 || S <= 0 || R <= 0 || pad < 0) return MIL_ERR_ARG;
    if (xs && ((R & 1) || (reinterpret_cast<uintptr_t>(xs) & 15))) return MIL_ERR_UNSUPPORTED;      // 2x2 blocks, 16-byte records
    if (T == 0) return MIL_OK;
    PrepArgs a{};
    a.rois = rois; a.params = params; a.bounds = bounds_dev; a.kk = kk_dev; a.out = out; a.xs = static_cast<__bf16*>(xs); a.out_u8 = out_u8;
    a.T = T; a.S = S; a.pad = params ? pad : 0; a.R = R; a.ksize = prep_ksize(S, R);
    int nri_max = 0;
    for (int r0 = 0; r0 < R; r0 += PREP_BAND) {
        const int r1 = r0 + PREP_BAND < R ? r0 + PREP_BAND : R;
        const int n = bounds_host[2 * (r1 - 1)] + bounds_host[2 * (r1 - 1) + 1] - bounds_host[2 * r0];
        if (n > nri_max) nri_max = n;
    }
    a.margin = (3 * a.pad + 15) & ~15;
    a.row_pitch = (a.margin + S * 3 + 3 * a.pad + 3 * 32 + 8 + (win ? 16 : 0) + 15) & ~15;       // + slack read behind the last window (+ a row's phase)
    a.lds_h_off = PREP_ROWS * a.row_pitch;
    a.lds_k_off = (a.lds_h_off + nri_max * R * 3 + 15) & ~15;
    a.lds_b_off = a.lds_k_off + R * a.ksize * 4;
    const int lds = a.lds_b_off + 2 * R * 4;
    if (lds > 160 * 1024 || T > 65535 || a.ksize > 32) return MIL_ERR_UNSUPPORTED;
    auto kern = a.ksize <= 4 ? tile_preprocess_kernel<4, false> : a.ksize <= 8 ? tile_preprocess_kernel<8, false>
              : a.ksize <= 12 ? tile_preprocess_kernel<12, false> : a.ksize <= 16 ? tile_preprocess_kernel<16, false>
              : a.ksize <= 24 ? tile_preprocess_kernel<24, false> : tile_preprocess_kernel<32, false>;
    if (win) {
        // 32-bit offsets inside a workgroup's descriptor: the rows of a band (+ the phase row) * pitch + one row below 2 GiB
        if (((int64_t)nri_max + 1) * win->row_pitch + 3 * (int64_t)S + 64 > (int64_t)0x7fff0000) return MIL_ERR_UNSUPPORTED;
        const uintptr_t bp = reinterpret_cast<uintptr_t>(win->base);
        a.delta = (int)(bp & 15);
        a.base_al = win->base - a.delta;
        a.total = ((int64_t)a.delta + win->base_bytes + 15) & ~(int64_t)15;
        a.src_pitch = win->row_pitch;
        a.win_off = reinterpret_cast<const long long*>(win->win_off);
        kern = a.ksize <= 4 ? tile_preprocess_kernel<4, true> : a.ksize <= 8 ? tile_preprocess_kernel<8, true>
             : a.ksize <= 12 ? tile_preprocess_kernel<12, true> : a.ksize <= 16 ? tile_preprocess_kernel<16, true>
             : a.ksize <= 24 ? tile_preprocess_kernel<24, true> : tile_preprocess_kernel<32, true>;
    }
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return MIL_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3((R + PREP_BAND - 1) / PREP_BAND, T), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_tile_preprocess(const uint8_t* rois, const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                                   const int32_t* kk_dev, float* out, int T, int S, int pad, int R, void* stream) {
    if (!out) return MIL_ERR_ARG;
    return prep_entry(rois, nullptr, params, bounds_host, bounds_dev, kk_dev, out, nullptr, nullptr, T, S, pad, R, stream);
}

// The same chain with the output left as bytes: out [T,3,R,R] uint8, planar — what Pillow's resize returns, before ToTensor +
// Normalize (RoiBuilder.py:193-210).  The uint8 feed of the stem kernels (mil_stem_fwd_fused_u8 / mil_stem_bwd_fused_u8 /
// mil_stem_s2d_u8) decodes it to exactly mil_tile_preprocess's fp32 values, in every compute mode.  Any R.
extern "C" int mil_tile_preprocess_u8(const uint8_t* rois, const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                                      const int32_t* kk_dev, uint8_t* out, int T, int S, int pad, int R, void* stream) {
    if (!out) return MIL_ERR_ARG;
    return prep_entry(rois, nullptr, params, bounds_host, bounds_dev, kk_dev, nullptr, nullptr, out, T, S, pad, R, stream);
}

// The same chain with the output written as the bf16 space-to-depth NHWC tensor xs [T,R/2,R/2,16] the stem kernels read
// (mil_stem_fwd_fused_xs / mil_stem_bwd_fused): a pre-processed bag then never exists as fp32 — the values are the bf16
// roundings of mil_tile_preprocess's, i.e. exactly what the stem's own fp32 -> bf16 conversion produces.  R must be even.
extern "C" int mil_tile_preprocess_s2d(const uint8_t* rois, const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                                       const int32_t* kk_dev, void* xs, int T, int S, int pad, int R, void* stream) {
    if (!xs) return MIL_ERR_ARG;
    return prep_entry(rois, nullptr, params, bounds_host, bounds_dev, kk_dev, nullptr, xs, nullptr, T, S, pad, R, stream);
}

// The three entries again for ROIs that are windows of a larger image left where it is (array_read_region, RoiBuilder.py:117-124,
// followed by the chains of :193-210): row y of window t starts at byte win_off_dev[t] + y * row_pitch of `base` (base_bytes
// long), at any alignment — the source convention of mil_roi_stats; win_off_dev [T] int64 on the device.  Everything else
// as above; a window's result is bit for bit the one the stack entry returns for the same pixels.
extern "C" int mil_tile_preprocess_win(const uint8_t* base, int64_t base_bytes, const int64_t* win_off_dev, int64_t row_pitch,
                                       const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                                       const int32_t* kk_dev, float* out, int T, int S, int pad, int R, void* stream) {
    if (!out) return MIL_ERR_ARG;
    const PrepWin w{base, base_bytes, win_off_dev, row_pitch};
    return prep_entry(nullptr, &w, params, bounds_host, bounds_dev, kk_dev, out, nullptr, nullptr, T, S, pad, R, stream);
}

extern "C" int mil_tile_preprocess_win_u8(const uint8_t* base, int64_t base_bytes, const int64_t* win_off_dev, int64_t row_pitch,
                                          const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                                          const int32_t* kk_dev, uint8_t* out, int T, int S, int pad, int R, void* stream) {
    if (!out) return MIL_ERR_ARG;
    const PrepWin w{base, base_bytes, win_off_dev, row_pitch};
    return prep_entry(nullptr, &w, params, bounds_host, bounds_dev, kk_dev, nullptr, nullptr, out, T, S, pad, R, stream);
}

extern "C" int mil_tile_preprocess_win_s2d(const uint8_t* base, int64_t base_bytes, const int64_t* win_off_dev, int64_t row_pitch,
                                           const int32_t* params, const int32_t* bounds_host, const int32_t* bounds_dev,
                                           const int32_t* kk_dev, void* xs, int T, int S, int pad, int R, void* stream) {
    if (!xs) return MIL_ERR_ARG;
    const PrepWin w{base, base_bytes, win_off_dev, row_pitch};
    return prep_entry(nullptr, &w, params, bounds_host, bounds_dev, kk_dev, nullptr, xs, nullptr, T, S, pad, R, stream);
}
