// Rotation / affine augmentation on the device: torchvision's RandomAffine / RandomRotation as its PIL backend computes them,
//     img.transform(size, Image.AFFINE, m, Image.BILINEAR, fillcolor=fill)
// bit for bit Pillow's bytes (libImaging/Geometry.c: affine_transform + bilinear_filter32RGB).  m = a0..a5 maps OUTPUT pixel
// centres to INPUT coordinates.  For a source of W x H pixels, output pixel (x, y), every channel:
//     xs = x + 0.5 ; ys = y + 0.5
//     xin = (a0*xs + a1*ys) + a2          yin = (a3*xs + a4*ys) + a5
//     not (0 <= xin < W and 0 <= yin < H):  out = fill
//     xf = xin - 0.5 ; yf = yin - 0.5 ; X = floor(xf) ; Y = floor(yf) ; dx = xf - X ; dy = yf - Y
//     x0 = clip(X, 0, W-1) ; x1 = clip(X+1, 0, W-1) ; y0 = clip(Y, 0, H-1)
//     v1 = p[y0][x0] + (p[y0][x1] - p[y0][x0]) * dx
//     v2 = p[Y+1][x0] + (p[Y+1][x1] - p[Y+1][x0]) * dx   if Y+1 < H   else v1            (Y >= -1 always)
//     out = (uint8) trunc( v1 + (v2 - v1) * dy )
// IEEE double, every product, sum and difference rounded once, in the order written: rounded.cuh, nothing fuses.  The byte
// differences are exact in double, and v1 + (v2 - v1) * dy never leaves [min, max] of its ends, so the truncation needs no clip.
// Where Y+1 is no row, the kernel reads row y0 twice: the same operations on the same bytes give v2 == v1 without a branch.
// A NaN coordinate (a finite matrix cannot make one from these sizes) counts as outside.
//
// ONE kernel for both layouts: the source is addressed by runtime tile / row / pixel / channel strides (64-bit products: a slide
// exceeds 2^31 bytes), the destination, a dense stack of n tiles of 3 * ow * oh bytes, by its pixel and channel strides:
//     planar       U8Tiles [n,3,h,w] -> [n,3,oh,ow]     src tile 3hw, row w, pixel 1, channel hw;   dst pixel 1, channel ow*oh
//     interleaved  ROI stack [n,S,S,3] -> [n,S,S,3]     src tile 3SS, row 3S, pixel 3, channel 1;   dst pixel 3, channel 1
//     slide        [H,W,3] -> windows [n,S,S,3]         src tile 0 (EVERY window reads the same image; the host folded the
//                                                       window's origin into a2, a5), row 3W, pixel 3, channel 1
// A thread owns four consecutive output pixels of a tile (row-major, a group may cross a row end): coordinates, weights, the
// inside test and the four tap offsets once per pixel, shared by the three channels; the twelve bytes leave as one dword per
// plane (planar) or as three consecutive dwords (interleaved) at whatever byte alignment the tile has (global memory takes
// unaligned dwords); the last, partial group of a tile is written byte by byte, and so is any other destination layout.  No
// access leaves the source image or the destination tile.  No LDS.
#include "common.cuh"
#include "rounded.cuh"

#define AF_THREADS 256
#define AF_PIX (AF_THREADS * 4)                         // output pixels per workgroup
#define AF_MAX_PIX (2147483647 - AF_PIX)                // ow * oh: the pixel index stays an int

struct AffineArgs {
    const uint8_t* src;
    uint8_t* dst;                   // [n, 3 * ow * oh] of this launch
    const double* mat;              // [n,6] of this launch
    long long src_tile, src_row, src_pix, src_chan;     // bytes
    long long dst_pix, dst_chan;
    int W, H, ow, oh;
    unsigned fill;                  // r | g << 8 | b << 16
};

__global__ __launch_bounds__(AF_THREADS) void affine_u8_kernel(AffineArgs a) {
    const int t = blockIdx.y, n = a.ow * a.oh;
    const int i = (blockIdx.x * AF_THREADS + threadIdx.x) * 4;
    if (i >= n) return;
    const int cnt = min(4, n - i);
    const double* const m = a.mat + 6 * (size_t)t;
    const double a0 = m[0], a1 = m[1], a2 = m[2], a3 = m[3], a4 = m[4], a5 = m[5];
    const double dW = (double)a.W, dH = (double)a.H;
    const uint8_t* const s = a.src + (long long)t * a.src_tile;
    int y = i / a.ow, x = i - y * a.ow;
    unsigned w[3] = {0u, 0u, 0u};                                       // four bytes of each channel
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < cnt) {
            const double xs = (double)x + 0.5, ys = (double)y + 0.5;    // exact
            const double xin = rn_dadd(rn_dadd(rn_dmul(a0, xs), rn_dmul(a1, ys)), a2);
            const double yin = rn_dadd(rn_dadd(rn_dmul(a3, xs), rn_dmul(a4, ys)), a5);
            if (xin >= 0.0 && xin < dW && yin >= 0.0 && yin < dH) {
                const double xf = rn_dsub(xin, 0.5), yf = rn_dsub(yin, 0.5);
                const double fx = __builtin_floor(xf), fy = __builtin_floor(yf);
                const double dx = rn_dsub(xf, fx), dy = rn_dsub(yf, fy);
                const int X = (int)fx, Y = (int)fy;                     // -1 .. W-1, -1 .. H-1
                const int x0 = max(X, 0), x1 = min(X + 1, a.W - 1), y0 = max(Y, 0), y1 = Y + 1 < a.H ? Y + 1 : y0;
                const long long r0 = (long long)y0 * a.src_row, r1 = (long long)y1 * a.src_row;
                const long long c0 = (long long)x0 * a.src_pix, c1 = (long long)x1 * a.src_pix;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* const p = s + (long long)c * a.src_chan;
                    const int p00 = p[r0 + c0], p01 = p[r0 + c1], p10 = p[r1 + c0], p11 = p[r1 + c1];
                    const double v1 = rn_dadd((double)p00, rn_dmul((double)(p01 - p00), dx));
                    const double v2 = rn_dadd((double)p10, rn_dmul((double)(p11 - p10), dx));
                    const double v = rn_dadd(v1, rn_dmul(rn_dsub(v2, v1), dy));
                    w[c] |= (unsigned)(int)v << (8 * q);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) w[c] |= ((a.fill >> (8 * c)) & 255u) << (8 * q);
            }
            if (++x == a.ow) { x = 0; ++y; }
        }
    }
    uint8_t* const d = a.dst + (long long)t * 3 * (long long)n;
    if (cnt == 4 && a.dst_pix == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_memcpy(d + (long long)c * a.dst_chan + i, &w[c], 4);
    } else if (cnt == 4 && a.dst_pix == 3 && a.dst_chan == 1) {
        unsigned o[3];                                                  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        o[0] = (w[0] & 255u) | ((w[1] & 255u) << 8) | ((w[2] & 255u) << 16) | (((w[0] >> 8) & 255u) << 24);
        o[1] = ((w[1] >> 8) & 255u) | (((w[2] >> 8) & 255u) << 8) | (((w[0] >> 16) & 255u) << 16) | (((w[1] >> 16) & 255u) << 24);
        o[2] = ((w[2] >> 16) & 255u) | ((w[0] >> 24) << 8) | ((w[1] >> 24) << 16) | ((w[2] >> 24) << 24);
        __builtin_memcpy(d + 3 * (long long)i, o, 12);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < cnt) {
#pragma unroll
                for (int c = 0; c < 3; ++c) d[(long long)(i + q) * a.dst_pix + (long long)c * a.dst_chan] = (uint8_t)(w[c] >> (8 * q));
            }
    }
}

// Pillow's bilinear affine transform of n uint8 images; include/mil_hip.h has the contract.  Everything that can be refused is
// refused here, on the host, before any GPU call.
extern "C" int mil_affine_u8(const uint8_t* src, int64_t src_tile_stride, int64_t src_row_stride, int64_t src_pix_stride,
                             int64_t src_chan_stride, int W, int H, uint8_t* dst, int64_t dst_pix_stride, int64_t dst_chan_stride,
                             int ow, int oh, const double* matrices, uint32_t fill_rgb, int n, void* stream) {
    if (!src || !dst || !matrices || n < 0 || W < 1 || H < 1 || ow < 1 || oh < 1) return MIL_ERR_ARG;
    if (src_tile_stride < 0 || src_row_stride < 1 || src_pix_stride < 1 || src_chan_stride < 1 || dst_pix_stride < 1 ||
        dst_chan_stride < 1)
        return MIL_ERR_ARG;
    if ((long long)ow * oh > AF_MAX_PIX) return MIL_ERR_UNSUPPORTED;
    if (n == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AffineArgs a{};
    a.src_tile = src_tile_stride; a.src_row = src_row_stride; a.src_pix = src_pix_stride; a.src_chan = src_chan_stride;
    a.dst_pix = dst_pix_stride; a.dst_chan = dst_chan_stride;
    a.W = W; a.H = H; a.ow = ow; a.oh = oh;
    a.fill = fill_rgb & 0xFFFFFFu;
    const int npix = ow * oh;
    const int split = (npix + AF_PIX - 1) / AF_PIX;
    for (int done = 0; done < n; done += 65535) {               // grid.y limit
        const int k = n - done < 65535 ? n - done : 65535;
        a.src = src + (long long)done * src_tile_stride;
        a.dst = dst + (long long)done * 3 * (long long)npix;
        a.mat = matrices + 6 * (size_t)done;
        hipLaunchKernelGGL(affine_u8_kernel, dim3(split, k), dim3(AF_THREADS), 0, st, a);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

// Elastic deformation fused into the same resampling: a per-tile control lattice ctrl [n,2,ly,lx]
// (doubles; component 0 the x displacement, 1 the y displacement, in SOURCE pixels; ly = gy + 3, lx = gx + 3 for an output divided
// into gy x gx cells) is evaluated as a uniform cubic B-spline through separable tables — iy [oh] / wy [oh,4] for the rows,
// ix [ow] / wx [ow,4] for the columns — and added to the affine coordinate before the inside test.  With c = ctrl[t][k]:
//     r_i = ((wy[y][0]*c[iy[y]+0][ix[x]+i] + wy[y][1]*c[iy[y]+1][ix[x]+i]) + wy[y][2]*c[iy[y]+2][ix[x]+i]) + wy[y][3]*c[iy[y]+3][ix[x]+i]
//     d   = ((wx[x][0]*r_0 + wx[x][1]*r_1) + wx[x][2]*r_2) + wx[x][3]*r_3                      dx for k = 0, dy for k = 1
//     xin = ((a0*xs + a1*ys) + a2) + dx          yin = ((a3*xs + a4*ys) + a5) + dy
// and from xin, yin on the contract above, word for word; every product and sum rounded once in the order written.  A zero
// lattice adds +0.0 or -0.0: neither the inside test nor a tap moves, the bytes are affine_u8_kernel's.  The kernel is written out
// in full beside affine_u8_kernel, whose text and code object stay as they were: same thread layout, strides and store paths.
// The eight column sums r_i depend on (y, ix[x]) only; a thread's four pixels share a row unless the group crosses a row end and
// share ix[x] unless it crosses a cell boundary, so they are computed for the first pixel (32 lattice loads, 8 table loads) and
// again only when either changes — the same operations on the same values, the same bits.  The lattice (a few KB per tile) and
// the tables are read from global memory: neighbouring threads read the same addresses.  The table indices are clamped to
// [0, ly-4] / [0, lx-4] (valid tables already lie there: the host checks them), so no access leaves the lattice.  No LDS.
struct ElasticArgs {
    AffineArgs af;
    const double* ctrl;             // [n,2,ly,lx] of this launch
    const int* iy;                  // [oh]
    const double* wy;               // [oh,4]
    const int* ix;                  // [ow]
    const double* wx;               // [ow,4]
    int ly, lx;
};

__global__ __launch_bounds__(AF_THREADS) void affine_elastic_u8_kernel(ElasticArgs e) {
    const AffineArgs& a = e.af;
    const int t = blockIdx.y, n = a.ow * a.oh;
    const int i = (blockIdx.x * AF_THREADS + threadIdx.x) * 4;
    if (i >= n) return;
    const int cnt = min(4, n - i);
    const double* const m = a.mat + 6 * (size_t)t;
    const double a0 = m[0], a1 = m[1], a2 = m[2], a3 = m[3], a4 = m[4], a5 = m[5];
    const double dW = (double)a.W, dH = (double)a.H;
    const uint8_t* const s = a.src + (long long)t * a.src_tile;
    const long long plane = (long long)e.ly * e.lx;                    // doubles per lattice component
    const double* const cx = e.ctrl + (long long)t * 2 * plane;
    int y = i / a.ow, x = i - y * a.ow;
    unsigned w[3] = {0u, 0u, 0u};                                       // four bytes of each channel
    double rx0 = 0.0, rx1 = 0.0, rx2 = 0.0, rx3 = 0.0, ry0 = 0.0, ry1 = 0.0, ry2 = 0.0, ry3 = 0.0;
    int cell = -1;                                                      // ix of the column sums held; -1: none (a new row too)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < cnt) {
            const int jx = min(max(e.ix[x], 0), e.lx - 4);
            if (jx != cell) {
                const int jy = min(max(e.iy[y], 0), e.ly - 4);
                const double* const v = e.wy + 4 * (long long)y;
                const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
                const double* const c0 = cx + (long long)jy * e.lx + jx;
                const double* const c1 = c0 + e.lx;
                const double* const c2 = c1 + e.lx;
                const double* const c3 = c2 + e.lx;
#define EL_COL(p, k) rn_dadd(rn_dadd(rn_dadd(rn_dmul(v0, c0[(p) + (k)]), rn_dmul(v1, c1[(p) + (k)])), rn_dmul(v2, c2[(p) + (k)])), \
                             rn_dmul(v3, c3[(p) + (k)]))
                rx0 = EL_COL(0, 0); rx1 = EL_COL(0, 1); rx2 = EL_COL(0, 2); rx3 = EL_COL(0, 3);
                ry0 = EL_COL(plane, 0); ry1 = EL_COL(plane, 1); ry2 = EL_COL(plane, 2); ry3 = EL_COL(plane, 3);
#undef EL_COL
                cell = jx;
            }
            const double* const u = e.wx + 4 * (long long)x;
            const double u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3];
            const double ddx = rn_dadd(rn_dadd(rn_dadd(rn_dmul(u0, rx0), rn_dmul(u1, rx1)), rn_dmul(u2, rx2)), rn_dmul(u3, rx3));
            const double ddy = rn_dadd(rn_dadd(rn_dadd(rn_dmul(u0, ry0), rn_dmul(u1, ry1)), rn_dmul(u2, ry2)), rn_dmul(u3, ry3));
            const double xs = (double)x + 0.5, ys = (double)y + 0.5;    // exact
            const double xin = rn_dadd(rn_dadd(rn_dadd(rn_dmul(a0, xs), rn_dmul(a1, ys)), a2), ddx);
            const double yin = rn_dadd(rn_dadd(rn_dadd(rn_dmul(a3, xs), rn_dmul(a4, ys)), a5), ddy);
            if (xin >= 0.0 && xin < dW && yin >= 0.0 && yin < dH) {
                const double xf = rn_dsub(xin, 0.5), yf = rn_dsub(yin, 0.5);
                const double fx = __builtin_floor(xf), fy = __builtin_floor(yf);
                const double dx = rn_dsub(xf, fx), dy = rn_dsub(yf, fy);
                const int X = (int)fx, Y = (int)fy;                     // -1 .. W-1, -1 .. H-1
                const int x0 = max(X, 0), x1 = min(X + 1, a.W - 1), y0 = max(Y, 0), y1 = Y + 1 < a.H ? Y + 1 : y0;
                const long long r0 = (long long)y0 * a.src_row, r1 = (long long)y1 * a.src_row;
                const long long c0 = (long long)x0 * a.src_pix, c1 = (long long)x1 * a.src_pix;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* const p = s + (long long)c * a.src_chan;
                    const int p00 = p[r0 + c0], p01 = p[r0 + c1], p10 = p[r1 + c0], p11 = p[r1 + c1];
                    const double v1 = rn_dadd((double)p00, rn_dmul((double)(p01 - p00), dx));
                    const double v2 = rn_dadd((double)p10, rn_dmul((double)(p11 - p10), dx));
                    const double v = rn_dadd(v1, rn_dmul(rn_dsub(v2, v1), dy));
                    w[c] |= (unsigned)(int)v << (8 * q);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) w[c] |= ((a.fill >> (8 * c)) & 255u) << (8 * q);
            }
            if (++x == a.ow) { x = 0; ++y; cell = -1; }
        }
    }
    uint8_t* const d = a.dst + (long long)t * 3 * (long long)n;
    if (cnt == 4 && a.dst_pix == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_memcpy(d + (long long)c * a.dst_chan + i, &w[c], 4);
    } else if (cnt == 4 && a.dst_pix == 3 && a.dst_chan == 1) {
        unsigned o[3];                                                  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        o[0] = (w[0] & 255u) | ((w[1] & 255u) << 8) | ((w[2] & 255u) << 16) | (((w[0] >> 8) & 255u) << 24);
        o[1] = ((w[1] >> 8) & 255u) | (((w[2] >> 8) & 255u) << 8) | (((w[0] >> 16) & 255u) << 16) | (((w[1] >> 16) & 255u) << 24);
        o[2] = ((w[2] >> 16) & 255u) | ((w[0] >> 24) << 8) | ((w[1] >> 24) << 16) | ((w[2] >> 24) << 24);
        __builtin_memcpy(d + 3 * (long long)i, o, 12);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < cnt) {
#pragma unroll
                for (int c = 0; c < 3; ++c) d[(long long)(i + q) * a.dst_pix + (long long)c * a.dst_chan] = (uint8_t)(w[c] >> (8 * q));
            }
    }
}

// mil_affine_u8 with a per-image control lattice; include/mil_hip.h has the contract.  Everything that can be refused is refused
// here, on the host, before any GPU call.  The lattice pointer advances with the matrices from launch to launch.
extern "C" int mil_affine_elastic_u8(const uint8_t* src, int64_t src_tile_stride, int64_t src_row_stride, int64_t src_pix_stride,
                                     int64_t src_chan_stride, int W, int H, uint8_t* dst, int64_t dst_pix_stride,
                                     int64_t dst_chan_stride, int ow, int oh, const double* matrices, uint32_t fill_rgb, int n,
                                     const double* ctrl, int ly, int lx, const int32_t* iy, const double* wy, const int32_t* ix,
                                     const double* wx, void* stream) {
    if (!src || !dst || !matrices || n < 0 || W < 1 || H < 1 || ow < 1 || oh < 1) return MIL_ERR_ARG;
    if (!ctrl || !iy || !wy || !ix || !wx || ly < 4 || lx < 4) return MIL_ERR_ARG;
    if (src_tile_stride < 0 || src_row_stride < 1 || src_pix_stride < 1 || src_chan_stride < 1 || dst_pix_stride < 1 ||
        dst_chan_stride < 1)
        return MIL_ERR_ARG;
    if ((long long)ow * oh > AF_MAX_PIX) return MIL_ERR_UNSUPPORTED;
    if (n == 0) return MIL_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ElasticArgs e{};
    AffineArgs& a = e.af;
    a.src_tile = src_tile_stride; a.src_row = src_row_stride; a.src_pix = src_pix_stride; a.src_chan = src_chan_stride;
    a.dst_pix = dst_pix_stride; a.dst_chan = dst_chan_stride;
    a.W = W; a.H = H; a.ow = ow; a.oh = oh;
    a.fill = fill_rgb & 0xFFFFFFu;
    e.iy = iy; e.wy = wy; e.ix = ix; e.wx = wx; e.ly = ly; e.lx = lx;
    const int npix = ow * oh;
    const int split = (npix + AF_PIX - 1) / AF_PIX;
    const size_t lattice = 2 * (size_t)ly * (size_t)lx;                // doubles per image
    for (int done = 0; done < n; done += 65535) {               // grid.y limit
        const int k = n - done < 65535 ? n - done : 65535;
        a.src = src + (long long)done * src_tile_stride;
        a.dst = dst + (long long)done * 3 * (long long)npix;
        a.mat = matrices + 6 * (size_t)done;
        e.ctrl = ctrl + lattice * (size_t)done;
        hipLaunchKernelGGL(affine_elastic_u8_kernel, dim3(split, k), dim3(AF_THREADS), 0, st, e);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}
