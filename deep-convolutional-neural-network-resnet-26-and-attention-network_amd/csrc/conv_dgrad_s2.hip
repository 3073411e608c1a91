// Data gradient of a stage-entry block's input (bf16 path): the transposed 3x3 stride-2 conv of dz1 PLUS the
// transposed 1x1 stride-2 projection of dz, times the lrelu' mask of the block input — one pass
// (reference: autograd of nnBlocks.py:175-189 for the blocks built at gbm/model.py:37-41).
//
// The zero-insert form (conv_igemm with zero_insert=1) stages a halo tile that is 3/4 zeros, multiplies all 9
// taps against it, and needs a second launch plus a full-resolution temporary for the projection.  Here the 256
// output pixels of a tile are split by parity class (py,px) = (y&1, x&1): each class is a 1/2/2/4-tap conv over
// the COMPACT dz map (geom.cuh: mil_s2_group), so the LDS tile is 81 pixels instead of 324, the MFMA work drops
// from 9 to 2.25 taps per output pixel, and the projection is 5..10 more K-groups of class (0,0) read from a
// second compact tile.  Wave w owns row tile w (16 pixels) of every class; the paired 16-byte register epilogue
// of the persistent conv kernel then stores two horizontally adjacent output pixels per lane pair.
#include "pf_common.cuh"

template <typename T>
struct DgradS2Args {
    const typename T::elem* dz1;      // [n,h,w,CZ]   gradient of the 3x3/s2 conv's output
    const typename T::elem* dz2;      // [n,h,w,CZ]   gradient of the block output (input of the projection's transposed conv), or null
    const typename T::elem* w;        // MIL_PACK_DGRAD_S2 fragments [mil_s2_nsteps][NT][64][8] (F32S: [hi | lo] pairs)
    const typename T::elem* act;      // [n,H,W,CXP]  block input (lrelu' mask), or null
    typename T::elem* y;              // [n,H,W,CXP]
    ConvGeom g;             // output tiling: Ho=H, Wo=W (dx), H=h, W=w (dz)
    int ch, cw;             // compact halo extent per image: TH/2+1, TW/2+1
    int lds_z2_off, lds_w_off;
    float slope;
    int ypx;                // bytes per pixel of y: CXP*ESZ, or 40 / 80 when a 20-channel output is written dense (MIL_DT_BF16_DGRAD / MIL_DT_F32S_DGRAD)
    unsigned act_bytes;
};

// T = BF16, or F32S (MIL_DT_F32S: fp32 tensors, bf16x3 split products — the compact tiles hold [hi | lo] planes, three MFMAs per
// fragment pair, fp32 mask / output; the 40 -> 24 channel entry only: the larger filters do not fit LDS beside two compact tiles).
// STREAM (split precision): the parity-class filter is NOT staged in LDS — every wave reads the packed fragments of a k-step
// from L1/L2 into registers two k-steps ahead (2 KB per wave-load and column tile, the fragment index in the scalar offset of
// the buffer load).  A [hi | lo] filter of 57 / 123 / 205 KB (40 -> 24, 64 -> 40, 80 -> 64 channels) beside two compact
// tiles left ONE 4-wave workgroup per CU (one wave per SIMD, matrix pipe 16 % busy: 0.52 ms) or did not fit at all (the two
// larger entries ran the zero-insert forms: 0.65 + 0.35 ms for a quarter of useful MFMAs); with only the compact tiles in
// LDS (29-54 KB) two to four workgroups are resident (80 channels: one, for its registers); the 64 -> 40 and 80 -> 64 channel
// entries run this form (the 40 -> 24 entry measured 0.60 ms streamed: it keeps the staged filter).
// NW = 8 (split precision, 40 -> 24 channels, maps of at least 16x32): 512-pixel output tiles (16 rows x 32 columns, compact
// tiles of 9x17 pixels) on eight waves that share ONE staged filter — two waves per SIMD instead of the one the 4-wave form
// is left with (57 KB filter + 252 VGPRs: matrix pipe 0.14 busy, 0.52 ms).
template <typename T, int CZ, int NT, bool STREAM = false, int NW = 4>
__global__ __launch_bounds__(64 * NW, (NW == 8 || (STREAM && CZ < 80) || (CZ <= 40 && !T::SPLIT)) ? 2 : 1) void conv_dgrad_s2_kernel(DgradS2Args<T> a, int ntiles, unsigned z_bytes, unsigned y_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MIL_POISON(smem);
    constexpr int ESZ = T::ESZ, FRAGB = 8 * ESZ;
    constexpr int CG = CZ / 8;
    constexpr int N16 = CZ * ESZ / 16;                       // 16-byte pieces per dz pixel
    constexpr int JB = T::SPLIT ? 8 : 16;
    constexpr int PIXZ = mil_pix_pitch(CZ, ESZ);
    constexpr int CXP = mil_nt_to_cp(NT);
    constexpr int NS = mil_s2_nsteps(CG);
    constexpr int NTHR = 64 * NW;
    constexpr int NPZ = ((NW == 8 ? 153 : 144) * N16 + NTHR - 1) / NTHR;      // <= 144 compact halo pixels (16 images of 3x3); NW 8: 9x17
    constexpr bool LAST_PARTIAL = (CXP % 16) != 0;
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, gq = lane >> 4;
    char* ldsZ = smem;
    char* ldsW = smem + a.lds_w_off;
    if constexpr (!STREAM) mil_stage_filter(ldsW, a.w, NS * NT * 64 * FRAGB, tid, NTHR);
    const __amdgpu_buffer_rsrc_t rs_w = mil_rsrc(a.w, NS * NT * 64 * FRAGB);
    const __amdgpu_buffer_rsrc_t rs_z1 = mil_rsrc(a.dz1, z_bytes);
    const __amdgpu_buffer_rsrc_t rs_z2 = mil_rsrc(a.dz2, a.dz2 ? z_bytes : 0);
    const __amdgpu_buffer_rsrc_t rs_act = mil_rsrc(a.act, a.act ? a.act_bytes : 0);
    const __amdgpu_buffer_rsrc_t rs_y = mil_rsrc(a.y, y_bytes);
    const int CH = a.ch, CW = a.cw, h = g.H, w = g.W, H = g.Ho, W = g.Wo;
    const int TW = 1 << g.tw_log2, TH = 1 << g.th_log2;

    // ---- tile-invariant tables ---------------------------------------------------------------------
    int z_pos[NPZ], z_lds[NPZ], z_rel[NPZ];                  // compact halo pieces (same for both sources)
    {
        const int total = ((CH * CW) << g.ti_log2) * N16;
#pragma unroll
        for (int i = 0; i < NPZ; ++i) {
            const int idx = tid + NTHR * i;
            z_pos[i] = -1; z_lds[i] = 0; z_rel[i] = 0;
            if (idx < total) {
                const int p = idx / N16, j = idx - p * N16;
                const int cx = p % CW, t = p / CW, cy = t % CH, ti = t / CH;
                z_pos[i] = (ti << 20) | (cy << 10) | cx;
                z_lds[i] = p * PIXZ + j * JB;
                z_rel[i] = ((ti * h + cy) * w + cx) * (CZ * ESZ) + j * 16;
            }
        }
    }
    // class pixel of this lane: index wave*16 + r of the 64 (ti, i, j) positions; the same for all four classes
    const int cp = wave * 16 + r;
    const int cj = cp & (TW / 2 - 1), ci = (cp >> (g.tw_log2 - 1)) & (TH / 2 - 1), cti = cp >> (g.tw_log2 + g.th_log2 - 2);
    const int pixbase = ((cti * CH + ci) * CW + cj) * PIXZ;
    int toff[NS];
    {
        int s = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int sl = 0; sl < mil_s2_steps(c, CG); ++sl, ++s) {
                const S2Group gr = mil_s2_group(c, 4 * sl + gq, CG);
                toff[s] = gr.valid ? gr.src * a.lds_z2_off + (gr.di * CW + gr.dj) * PIXZ + gr.cg * 16 : 0;
            }
        }
    }
    // epilogue: after one v_permlane16_swap per accumulator register between classes 2p and 2p+1 a lane holds 8
    // consecutive channels (16*nt + 8*(gq>>1) ...) of output pixel (2i + p, 2j + (gq&1))
    int o_rel[2], o_pos[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int oy = 2 * ci + p, ox = 2 * cj + (gq & 1);
        o_rel[p] = (cti * H + oy) * W + ox;                      // in pixels: act is read at CXP*2 bytes per pixel, y written at a.ypx
        o_pos[p] = (cti << 20) | (oy << 10) | ox;
    }
    const bool last_ok = !LAST_PARTIAL || (gq >> 1) == 0;

    TileWalker cur, nxt;
    const int bid = mil_xcd_block_id();
    cur.init(g, bid, gridDim.x);
    nxt = cur; nxt.advance();
    auto fetch_z = [&](u32x4_t (&r1)[NPZ], u32x4_t (&r2)[NPZ], const TileOrigin& o) {
        const int i0 = o.oy0 >> 1, j0 = o.ox0 >> 1;
        const int base = ((o.img0 * h + i0) * w + j0) * (CZ * ESZ);
        const int ylim = h - i0, xlim = w - j0, ilim = g.n_img - o.img0;
#pragma unroll
        for (int i = 0; i < NPZ; ++i) {
            const int p = z_pos[i];
            const bool ok = p >= 0 && (p >> 20) < ilim && ((p >> 10) & 1023) < ylim && (p & 1023) < xlim;
            const unsigned off = ok ? (unsigned)(base + z_rel[i]) : MIL_OOB;
            r1[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_z1, off, 0, 0);
            r2[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_z2, off, 0, 0);
        }
    };
    constexpr int NE = T::SPLIT ? 2 : 1;                     // 16-byte loads per 8 channels of the mask operand
    auto fetch_epi = [&](const TileOrigin& o, unsigned (&ooff)[2], u32x4_t (&ract)[2][NT][NE]) {
        const int obase = (o.img0 * H + o.oy0) * W + o.ox0;
        const int ylim = H - o.oy0, xlim = W - o.ox0, ilim = g.n_img - o.img0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const bool ok = (o_pos[p] >> 20) < ilim && ((o_pos[p] >> 10) & 1023) < ylim && (o_pos[p] & 1023) < xlim;
            const int opix = obase + o_rel[p];
            ooff[p] = ok ? (unsigned)(opix * a.ypx + (gq >> 1) * 8 * ESZ) : MIL_OOB;
            const unsigned aoff = ok ? (unsigned)(opix * (CXP * ESZ) + (gq >> 1) * 8 * ESZ) : MIL_OOB;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const unsigned off = (LAST_PARTIAL && nt == NT - 1 && !last_ok) ? MIL_OOB : aoff + nt * 16 * ESZ;
                if (a.act) {
                    ract[p][nt][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_act, off, 0, 0);
                    if constexpr (T::SPLIT) ract[p][nt][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_act, off == MIL_OOB ? MIL_OOB : off + 16, 0, 0);
                }
            }
        }
    };

    // STREAM: no register prefetch of the next tile (its 18-24 pieces and the mask operands do not fit beside the streamed filter
    // fragments: the loads are issued at the top of the tile and behind the MFMA loop; the other resident workgroups cover them)
    // (80 channels, streamed: ONE wave per SIMD — 64 accumulator + 64 fragment registers beside 25 tap offsets do not fit 256 —
    // so the next tile IS prefetched in registers, as in the staged form)
    constexpr bool NOPF = STREAM && CZ < 80;
    u32x4_t rz1[NPZ], rz2[NPZ];
    unsigned ooff_n[2];
    u32x4_t ract_n[2][NT][NE];
    if (!NOPF && bid < ntiles) {
        fetch_z(rz1, rz2, cur.origin(g));
        fetch_epi(cur.origin(g), ooff_n, ract_n);
    }
    const int G = gridDim.x;
    for (int tile = bid; tile < ntiles; tile += G) {
        const TileOrigin o_cur = cur.origin(g);
        __syncthreads();                       // every wave has finished reading the compact tiles of the previous tile
        if constexpr (NOPF) fetch_z(rz1, rz2, o_cur);
#pragma unroll
        for (int i = 0; i < NPZ; ++i) {
            if (z_pos[i] >= 0) {
                mil_commit_piece<T, CZ * 2>(ldsZ + z_lds[i], rz1[i]);
                mil_commit_piece<T, CZ * 2>(ldsZ + a.lds_z2_off + z_lds[i], rz2[i]);
            }
        }
        unsigned ooff[2];
        u32x4_t ract[2][NT][NE];
        if constexpr (!NOPF) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            ooff[p] = ooff_n[p];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int e = 0; e < NE; ++e) ract[p][nt][e] = ract_n[p][nt][e];
        }
        }
        __syncthreads();
        if constexpr (!NOPF) {
        if (tile + G < ntiles) {
            fetch_z(rz1, rz2, nxt.origin(g));
            fetch_epi(nxt.origin(g), ooff_n, ract_n);
        }
        }
        cur = nxt; nxt.advance();

        f32x4_t acc[4][NT];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[c][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        {
            // one k-step ahead (the steps of the four parity classes flattened into one sequence): the fragments of step
            // s+1 are read before the MFMAs of step s and scheduling fences keep that order (see mil_conv_ring)
            auto cls = [](int st) { int c = 0; while (st >= mil_s2_steps(c, CG)) { st -= mil_s2_steps(c, CG); ++c; } return c; };
            constexpr int WD = (STREAM && NT < 4) ? 2 : 1, WR = WD + 1;      // filter fragments in flight: k-steps ahead / ring slots (8 VGPRs per split fragment)
            Frag8<T> xq[2], wq[WR][NT];
            auto wfrag = [&](int st, int nt) {
                if constexpr (STREAM) {                              // split precision only: [hi | lo] = two 16-byte loads per lane
                    Frag8<T> f;
                    f.h = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rs_w, (unsigned)(lane * FRAGB), (st * NT + nt) * 64 * FRAGB, 0));
                    f.l = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rs_w, (unsigned)(lane * FRAGB + 16), (st * NT + nt) * 64 * FRAGB, 0));
                    return f;
                } else {
                    return lds_frag<T>(ldsW + ((st * NT + nt) * 64 + lane) * FRAGB);
                }
            };
            xq[0] = lds_pix_frag<T, CZ * 2>(ldsZ + pixbase + toff[0]);
#pragma unroll
            for (int k = 0; k < WD && k < NS; ++k)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) wq[k % WR][nt] = wfrag(k, nt);
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                if (st + 1 < NS) xq[(st + 1) & 1] = lds_pix_frag<T, CZ * 2>(ldsZ + pixbase + toff[st + 1 < NS ? st + 1 : st]);
                if (st + WD < NS) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) wq[(st + WD) % WR][nt] = wfrag(st + WD, nt);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[cls(st)][nt] = mma8(wq[st % WR][nt], xq[st & 1], acc[cls(st)][nt]);          // D[channel][pixel]
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (NOPF) fetch_epi(o_cur, ooff, ract);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float lo = acc[2 * p][nt][i], hi = acc[2 * p + 1][nt][i];
                    if (i == 0) mil_swap16<true>(lo, hi); else mil_swap16<false>(lo, hi);
                    v[i] = lo;
                    v[4 + i] = hi;
                }
                const unsigned off = (LAST_PARTIAL && nt == NT - 1 && !last_ok) ? MIL_OOB : ooff[p] + nt * 16 * ESZ;
                if constexpr (T::SPLIT) {
                    if (a.act) {
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const f32x4_t t = __builtin_bit_cast(f32x4_t, ract[p][nt][e]);
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[4 * e + i] *= (t[i] > 0.f ? 1.f : a.slope);
                        }
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, f32x4_t{v[0], v[1], v[2], v[3]}), rs_y, off, 0, 0);
                    // dense 20-channel output (a.ypx = 80): channels 20-23 of the last column tile do not exist
                    const bool skip2 = off == MIL_OOB || (LAST_PARTIAL && nt == NT - 1 && a.ypx != CXP * ESZ);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, f32x4_t{v[4], v[5], v[6], v[7]}), rs_y, skip2 ? MIL_OOB : off + 16, 0, 0);
                } else {
                if (a.act) {
                    const bf16x8_t t = __builtin_bit_cast(bf16x8_t, ract[p][nt][0]);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] *= ((float)t[i] > 0.f ? 1.f : a.slope);
                }
                bf16x8_t ov;
#pragma unroll
                for (int i = 0; i < 8; ++i) ov[i] = (__bf16)v[i];
                const u32x4_t ou = __builtin_bit_cast(u32x4_t, ov);
                if (LAST_PARTIAL && nt == NT - 1 && a.ypx != CXP * 2) __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{ou[0], ou[1]}, rs_y, off, 0, 0);      // dense: channels 16-19 only
                else __builtin_amdgcn_raw_buffer_store_b128(ou, rs_y, off, 0, 0);
                }
            }
        }
    }
}

template <typename T, int CZ, int NT, bool STREAM = false, int NW = 4>
static int launch_dgrad_s2(DgradS2Args<T> a, hipStream_t st) {
    constexpr int ESZ = T::ESZ;
    constexpr int CG = CZ / 8, PIXZ = mil_pix_pitch(CZ, ESZ), CXP = mil_nt_to_cp(NT);
    if constexpr (NW == 8) mil_geom_set(a.g, 5, 4, 0);         // 16 x 32 output pixels of one image
    else
    mil_geom_tiles(a.g, 8);
    if (a.g.tw_log2 < 1 || a.g.th_log2 < 1) return MIL_ERR_UNSUPPORTED;
    a.ch = (1 << a.g.th_log2) / 2 + 1; a.cw = (1 << a.g.tw_log2) / 2 + 1;
    const int npx = (a.ch * a.cw) << a.g.ti_log2;
    if (npx > (NW == 8 ? 153 : 144)) return MIL_ERR_UNSUPPORTED;
    const int z_bytes = (npx * PIXZ + 15) & ~15;
    const int w_bytes = STREAM ? 0 : mil_s2_nsteps(CG) * NT * 64 * 8 * ESZ;
    a.lds_z2_off = z_bytes; a.lds_w_off = 2 * z_bytes;
    const int lds = 2 * z_bytes + w_bytes;
    if (lds > 160 * 1024) return MIL_ERR_UNSUPPORTED;
    auto kern = conv_dgrad_s2_kernel<T, CZ, NT, STREAM, NW>;
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return MIL_ERR_LAUNCH;
    const int per_cu = mil_resident_per_cu(kern, lds, 4, 64 * NW);      // by registers AND LDS (see conv_s2_entry.hip)
    const size_t z_img = (size_t)a.g.H * a.g.W * CZ * ESZ, act_img = (size_t)a.g.Ho * a.g.Wo * CXP * ESZ, y_img = (size_t)a.g.Ho * a.g.Wo * a.ypx;
    int chunk = mil_imgs_under_2g(z_img > act_img ? z_img : act_img);
    if (chunk >= 16) chunk &= ~15;
    const int n_total = a.g.n_img;
    for (int i0 = 0; i0 < n_total; i0 += chunk) {
        const int n = (n_total - i0 < chunk) ? n_total - i0 : chunk;
        DgradS2Args<T> c = a;
        c.g.n_img = n;
        c.g.n_groups = (n + (1 << c.g.ti_log2) - 1) >> c.g.ti_log2;
        c.dz1 = a.dz1 + (size_t)i0 * (z_img / ESZ);
        if (a.dz2) c.dz2 = a.dz2 + (size_t)i0 * (z_img / ESZ);
        if (a.act) c.act = a.act + (size_t)i0 * (act_img / ESZ);
        c.act_bytes = (unsigned)(act_img * n);
        c.y = a.y + (size_t)i0 * (y_img / ESZ);
        const int ntiles = c.g.n_groups * c.g.tiles_y * c.g.tiles_x;
        int grid = mil_num_cus() * per_cu;
        if (grid > ntiles) grid = ntiles;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, st, c, ntiles, (unsigned)(z_img * n), (unsigned)(y_img * n));
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

// y[n,H,W,cx_p] = lrelu'(act) * ( conv3x3_s2^T(dz1) + conv1x1_s2^T(dz2) ), with wpack from
// mil_pack_conv_weights(mode MIL_PACK_DGRAD_S2: w = the 3x3 weight, bias argument = the 1x1 projection weight or null).
// dz1/dz2 [n,h,w,cz_p] with h = (H-1)/2+1, w = (W-1)/2+1.  bf16, (cz_p,cx_p) in {(40,24),(64,40),(80,64)}; with
// MIL_DT_BF16_DGRAD and (40,24) y is [n,H,W,20] (dense gradient layout of the 20-channel layer; act stays padded).
extern "C" int mil_conv_dgrad_s2(const void* dz1, const void* dz2, const void* wpack, const void* act, void* y, int n_img,
                                 int h, int w, int cz_p, int H, int W, int cx_p, float slope, int dtype, void* stream) {
    if (!dz1 || !wpack || !y || n_img < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return MIL_ERR_ARG;
    if ((dtype != MIL_DT_BF16 && dtype != MIL_DT_BF16_DGRAD && dtype != MIL_DT_F32S && dtype != MIL_DT_F32S_DGRAD) || h != (H - 1) / 2 + 1 || w != (W - 1) / 2 + 1 || slope < 0.f || slope >= 1.f) return MIL_ERR_UNSUPPORTED;
    if (n_img == 0) return MIL_OK;
    if (dtype == MIL_DT_F32S || dtype == MIL_DT_F32S_DGRAD) {      // fp32 tensors, bf16x3 products: all three entries, the filter streamed
        // (80 -> 64 channels: 64 accumulator + 64 fragment registers beside 25 per-lane tap offsets spill 58 VGPRs at two waves per
        // SIMD, so that entry runs ONE wave per SIMD with the next tile prefetched in registers — against 0.34 ms on the
        // zero-insert form of the generic kernel)
        if (!((cz_p == 40 && cx_p == 24) || (cz_p == 64 && cx_p == 40) || (cz_p == 80 && cx_p == 64))) return MIL_ERR_UNSUPPORTED;
        if (dtype == MIL_DT_F32S_DGRAD && cz_p != 40) return MIL_ERR_UNSUPPORTED;
        DgradS2Args<F32S> b{};
        b.dz1 = (const float*)dz1; b.dz2 = (const float*)dz2; b.w = (const float*)wpack; b.act = (const float*)act; b.y = (float*)y;
        b.g.n_img = n_img; b.g.H = h; b.g.W = w; b.g.Ho = H; b.g.Wo = W; b.g.ks = 3; b.g.stride = 1; b.g.pad = 1; b.g.zins = 1;
        b.slope = slope; b.ypx = dtype == MIL_DT_F32S_DGRAD ? 80 : cx_p * 4;      // y [n,H,W,20] dense fp32, or padded
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        if (cz_p == 40) {               // staged filter: 0.52 ms against 0.60 ms streamed; eight waves on one staged filter where the map allows
            if (H >= 16 && W >= 32) return launch_dgrad_s2<F32S, 40, 2, false, 8>(b, st);
            return launch_dgrad_s2<F32S, 40, 2>(b, st);
        }
        if (cz_p == 64) return launch_dgrad_s2<F32S, 64, 3, true>(b, st);
        return launch_dgrad_s2<F32S, 80, 4, true>(b, st);
    }
    DgradS2Args<BF16> a{};
    a.dz1 = (const __bf16*)dz1; a.dz2 = (const __bf16*)dz2; a.w = (const __bf16*)wpack; a.act = (const __bf16*)act; a.y = (__bf16*)y;
    a.g.n_img = n_img; a.g.H = h; a.g.W = w; a.g.Ho = H; a.g.Wo = W; a.g.ks = 3; a.g.stride = 1; a.g.pad = 1; a.g.zins = 1;
    a.slope = slope;
    a.ypx = cx_p * 2;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MIL_DT_BF16_DGRAD) {            // y [n,H,W,20] dense: the 40 -> 20 channel entry only
        if (cz_p != 40 || cx_p != 24) return MIL_ERR_UNSUPPORTED;
        a.ypx = 40;
    }
    if (cz_p == 40 && cx_p == 24) return launch_dgrad_s2<BF16, 40, 2>(a, st);
    if (cz_p == 64 && cx_p == 40) return launch_dgrad_s2<BF16, 64, 3>(a, st);
    if (cz_p == 80 && cx_p == 64) return launch_dgrad_s2<BF16, 80, 4>(a, st);
    return MIL_ERR_UNSUPPORTED;
}

// ---------------------------------------------------------------------------------------------------------------------
// Stage-entry backward in ONE launch (bf16): conv_dgrad_s2_kernel's data gradient, unchanged, plus the weight gradients of
// the block's 3x3/s2 conv and 1x1/s2 projection and the conv's bias gradient — what wgrad_kernel<.., PROJ> computes in a
// second pass over the same three tensors.  Everything that pass reads is on chip here but the one-pixel top/left ring of
// the block input: the input is therefore staged as a tile of [pixel][channel] records, one row and one column more than the output tile (record (ry,rx) = input pixel
// (oy0 - 1 + ry, ox0 - 1 + rx), zero outside the image) instead of being loaded per lane for the mask, the mask is read back
// from that tile, and per tile the 32-pixel k-steps over the CENTRE pixels of the compact dz tiles (the halo row and
// column belong to the neighbouring tiles) feed
//     dW1[(tap,ci)][co] += sum_q x[2q + tap - 1][ci] * dz1[q][co],   dWp[ci][co] += sum_q x[2q][ci] * dz2[q][co],
//     db1[co] += sum_q dz1[q][co]
// with both operands read by ds_read_b64_tr_b16 (per-lane addresses: the stride-2 gather of x costs nothing extra).  The
// accumulators stay in registers over the workgroup's whole tile walk; at the end every workgroup writes ONE fp32 slab in
// the layout of wgrad_kernel<.., PROJ> (rows tap*cinp + ci, the bias row tile, the projection's row tiles behind it), so
// the same two MilReduceJobs finish the sums in fixed order.  No cross-workgroup communication.
// Output tiles of one image only (maps with a side above 8 pixels); LDS: [dz1 9x9][dz2 9x9][filter][x 17x17] (NW = 8: 9x17, 17x33).
// The weight gradients are mil_conv_wgrad_pair's BIT FOR BIT: this kernel walks the dz tiles of that kernel (8x8 pixels for
// the 40 -> 60 entry, 16x8 for 20 -> 40) in the same order, pixel p of a tile sits in the same k-step and the same MFMA k-slot
// in both, and the launcher below takes its grid — so every slab element is the same sequence of MFMAs.  (A training run
// amplifies last-bit gradient differences: 25 steps of the benchmark turn another summation order of ONE weight gradient
// into percent-size differences of every output.)
#include "reduce.cuh"

struct EntryBwdArgs {
    const __bf16* dz1;      // [n,h,w,CZ]
    const __bf16* dz2;      // [n,h,w,CZ]
    const __bf16* w;        // MIL_PACK_DGRAD_S2 fragments
    const __bf16* x;        // [n,H,W,CXP]  block input: weight-gradient operand and (masked) lrelu' mask
    __bf16* y;              // [n,H,W,CXP], or dense ([n,H,W,20], ypx = 40)
    float* slab;            // [gridDim.x][(MT + 1 + PMN) * 16][NTZ * 16]
    ConvGeom g;             // output tiling: Ho=H, Wo=W (dx), H=h, W=w (dz)
    int lds_z2_off, lds_w_off, lds_x_off;
    float slope;
    int ypx;                // bytes per pixel of y
    int masked;
};

// NW = 8 (the 20 -> 40 entry): 32x16-pixel output tiles = the 16x8 dz pixels of ONE 128-pixel tile of the pair kernel, on eight
// waves: in the data gradient wave w owns row w of the tile's 8 x 16 class pixels, and the weight-gradient phase runs the pair
// kernel's four k-steps — k-step ks = dz rows 2ks, 2ks+1 of 16 pixels — over the whole tile (row tiles w, w + 8).
// NW = 4: 16x16-pixel output tiles = its 64-pixel (8x8) dz tiles, two k-steps of four rows of 8.
template <int CZ, int NT, int NW>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void conv_entry_bwd_kernel(EntryBwdArgs a, int ntiles, unsigned z_bytes, unsigned x_bytes, unsigned y_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MIL_POISON(smem);
    using T = BF16;
    constexpr int CG = CZ / 8, N16 = CZ * 2 / 16, PIXZ = mil_pix_pitch(CZ, 2);
    constexpr int CXP = mil_nt_to_cp(NT), CGX = CXP / 8, X16 = CXP * 2 / 16, PIXB = mil_pix_pitch(CXP, 2);
    constexpr int NS = mil_s2_nsteps(CG);
    constexpr int NTHR = 64 * NW, CH = 9, CW = NW == 8 ? 17 : 9, XH = 17, XW = NW == 8 ? 33 : 17;
    constexpr int NPZ = (CH * CW * N16 + NTHR - 1) / NTHR, NPX = (XH * XW * X16 + NTHR - 1) / NTHR;
    constexpr bool LAST_PARTIAL = (CXP % 16) != 0;
    // weight-gradient GEMM: M = (tap, ci) in row groups of 8 channels, N = co, K = the tile's 64 centre dz pixels
    constexpr int RG = 9 * CGX, MT = (RG + 1) / 2, NTZ = (CZ + 15) / 16, MW = (MT + NW - 1) / NW;
    constexpr int PM0 = 2 * CGX, PM1 = (5 * CGX - 1) / 2, PMN = PM1 - PM0 + 1;      // row tiles holding centre-tap rows
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, gq = lane >> 4;
    char* ldsZ = smem;
    char* ldsW = smem + a.lds_w_off;
    char* ldsX = smem + a.lds_x_off;
    mil_stage_filter(ldsW, a.w, NS * NT * 64 * 16, tid, NTHR);
    const __amdgpu_buffer_rsrc_t rs_z1 = mil_rsrc(a.dz1, z_bytes);
    const __amdgpu_buffer_rsrc_t rs_z2 = mil_rsrc(a.dz2, z_bytes);
    const __amdgpu_buffer_rsrc_t rs_x = mil_rsrc(a.x, x_bytes);
    const __amdgpu_buffer_rsrc_t rs_y = mil_rsrc(a.y, y_bytes);
    const int h = g.H, w = g.W, H = g.Ho, W = g.Wo;

    // ---- tile-invariant tables: the pieces (16 bytes) of the compact dz tiles and of the x tile this thread moves ----
    int z_pos[NPZ], z_lds[NPZ], z_rel[NPZ];
#pragma unroll
    for (int i = 0; i < NPZ; ++i) {
        const int idx = tid + NTHR * i;
        z_pos[i] = -1; z_lds[i] = 0; z_rel[i] = 0;
        if (idx < CH * CW * N16) {
            const int p = idx / N16, j = idx - p * N16;
            const int cx = p % CW, cy = p / CW;
            z_pos[i] = (cy << 10) | cx;
            z_lds[i] = p * PIXZ + j * 16;
            z_rel[i] = (cy * w + cx) * (CZ * 2) + j * 16;
        }
    }
    int x_pos[NPX], x_lds[NPX], x_rel[NPX];
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        const int idx = tid + NTHR * i;
        x_pos[i] = -1; x_lds[i] = 0; x_rel[i] = 0;
        if (idx < XH * XW * X16) {
            const int p = idx / X16, j = idx - p * X16;
            const int rx = p % XW, ry = p / XW;
            x_pos[i] = (ry << 10) | rx;
            x_lds[i] = p * PIXB + j * 16;
            x_rel[i] = (ry * W + rx) * (CXP * 2) + j * 16;
        }
    }
    // data gradient: class pixel of this lane, index wave*16 + r of the 64 (i, j) positions, the same for all four classes
    const int cp = wave * 16 + r;
    const int cj = cp & (CW - 2), ci = cp >> (NW == 8 ? 4 : 3);
    const int pixbase = (ci * CW + cj) * PIXZ;
    int toff[NS];
    {
        int s = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int sl = 0; sl < mil_s2_steps(c, CG); ++sl, ++s) {
                const S2Group gr = mil_s2_group(c, 4 * sl + gq, CG);
                toff[s] = gr.valid ? gr.src * a.lds_z2_off + (gr.di * CW + gr.dj) * PIXZ + gr.cg * 16 : 0;
            }
        }
    }
    const bool last_ok = !LAST_PARTIAL || (gq >> 1) == 0;
    // weight gradient: lane (gq, q4, p4) reads 4 channels of pixel (row gq, column q4 / q4 + 4) of a k-step's 4 x 8 pixels
    const int q4 = r >> 2, p4 = r & 3;
    // (the pair kernel's pixel order: pixel 8*gq + q4 (+ 4) of a k-step's 32, row-major over a tile 8 or 16 pixels wide)
    const int krow = NW == 8 ? gq >> 1 : gq, kcol = (NW == 8 ? (gq & 1) * 8 : 0) + q4;
    const int zb = (krow * CW + kcol) * PIXZ + p4 * 8;
    const int xb = (2 * krow * XW + 2 * kcol) * PIXB + (p4 & 1) * 8;
    constexpr int KROWS = NW == 8 ? 2 : 4;      // dz rows per k-step
    int woff[MW];
    int proj_i = -1, proj_mt = 0;               // the owned row tile (at most one per wave) that also feeds the projection
#pragma unroll
    for (int i = 0; i < MW; ++i) {
        const int mt = wave + NW * i;
        if (mt < MT && mt >= PM0 && mt <= PM1) { proj_i = i; proj_mt = mt; }
        int rg = 2 * mt + (p4 >> 1);
        if (rg >= RG) rg = 0;                    // rows past the filter: finite duplicates, never read back
        const int tap = rg / CGX, cg = rg - tap * CGX;
        const int ky = tap / 3, kx = tap - ky * 3;
        woff[i] = (ky * XW + kx) * PIXB + cg * 16;
    }
    const bool bias_wave = wave == 0;
    f32x4_t wacc[MW][NTZ], waccb[NTZ], waccp[NTZ];
#pragma unroll
    for (int nt = 0; nt < NTZ; ++nt) {
        waccb[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        waccp[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < MW; ++i) wacc[i][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    bf16x8_t ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

    TileWalker cur, nxt;
    const int bid = mil_xcd_block_id();
    cur.init(g, bid, gridDim.x);
    nxt = cur; nxt.advance();
    u32x4_t rz1[NPZ], rz2[NPZ], rx[NPX];
    auto fetch = [&](const TileOrigin& o) {
        const int i0 = o.oy0 >> 1, j0 = o.ox0 >> 1;
        const int zbase = ((o.img0 * h + i0) * w + j0) * (CZ * 2);
        const int ylim = h - i0, xlim = w - j0;
#pragma unroll
        for (int i = 0; i < NPZ; ++i) {
            const int p = z_pos[i];
            const bool ok = p >= 0 && (p >> 10) < ylim && (p & 1023) < xlim;
            const unsigned off = ok ? (unsigned)(zbase + z_rel[i]) : MIL_OOB;
            rz1[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_z1, off, 0, 0);
            rz2[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_z2, off, 0, 0);
        }
        const int iy0 = o.oy0 - 1, ix0 = o.ox0 - 1;
        const int xbase = ((o.img0 * H + iy0) * W + ix0) * (CXP * 2);      // may be negative; valid lanes are not
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            const int p = x_pos[i];
            const bool ok = p >= 0 && (unsigned)(iy0 + (p >> 10)) < (unsigned)H && (unsigned)(ix0 + (p & 1023)) < (unsigned)W;
            rx[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? (unsigned)(xbase + x_rel[i]) : MIL_OOB, 0, 0);
        }
    };
    if (bid < ntiles) fetch(cur.origin(g));
    const int G = gridDim.x;
    for (int tile = bid; tile < ntiles; tile += G) {
        const TileOrigin o_cur = cur.origin(g);
        __syncthreads();                       // every wave has finished reading the three tiles of the previous step
#pragma unroll
        for (int i = 0; i < NPZ; ++i) {
            if (z_pos[i] >= 0) {
                *reinterpret_cast<u32x4_t*>(ldsZ + z_lds[i]) = rz1[i];
                *reinterpret_cast<u32x4_t*>(ldsZ + a.lds_z2_off + z_lds[i]) = rz2[i];
            }
        }
#pragma unroll
        for (int i = 0; i < NPX; ++i)
            if (x_pos[i] >= 0) *reinterpret_cast<u32x4_t*>(ldsX + x_lds[i]) = rx[i];
        __syncthreads();
        if (tile + G < ntiles) fetch(nxt.origin(g));
        cur = nxt; nxt.advance();

        // ---- data gradient: exactly conv_dgrad_s2_kernel's loop (same fragments, same MFMA order) ----
        f32x4_t acc[4][NT];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[c][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        {
            auto cls = [](int st) { int c = 0; while (st >= mil_s2_steps(c, CG)) { st -= mil_s2_steps(c, CG); ++c; } return c; };
            Frag8<T> xq[2], wq[2][NT];
            xq[0] = lds_pix_frag<T, CZ * 2>(ldsZ + pixbase + toff[0]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wq[0][nt] = lds_frag<T>(ldsW + (nt * 64 + lane) * 16);
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                if (st + 1 < NS) {
                    xq[(st + 1) & 1] = lds_pix_frag<T, CZ * 2>(ldsZ + pixbase + toff[st + 1 < NS ? st + 1 : st]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) wq[(st + 1) & 1][nt] = lds_frag<T>(ldsW + (((st + 1) * NT + nt) * 64 + lane) * 16);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[cls(st)][nt] = mma8(wq[st & 1][nt], xq[st & 1], acc[cls(st)][nt]);          // D[channel][pixel]
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // epilogue: one v_permlane16_swap per accumulator register between classes 2p and 2p+1, then a lane holds 8
        // consecutive channels (16*nt + 8*(gq>>1) ...) of output pixel (2i + p, 2j + (gq&1)); the mask comes from the x tile
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int oy = 2 * ci + p, ox = 2 * cj + (gq & 1);
            const bool ok = oy < H - o_cur.oy0 && ox < W - o_cur.ox0;
            const unsigned ooff = ok ? (unsigned)((((o_cur.img0 * H + o_cur.oy0 + oy) * W + o_cur.ox0 + ox)) * a.ypx + (gq >> 1) * 16) : MIL_OOB;
            const char* mrec = ldsX + ((oy + 1) * XW + ox + 1) * PIXB;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float v[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float lo = acc[2 * p][nt][i], hi = acc[2 * p + 1][nt][i];
                    if (i == 0) mil_swap16<true>(lo, hi); else mil_swap16<false>(lo, hi);
                    v[i] = lo;
                    v[4 + i] = hi;
                }
                const bool dead = LAST_PARTIAL && nt == NT - 1 && !last_ok;      // channels past the record: nothing stored
                const unsigned off = (dead || !ok) ? MIL_OOB : ooff + nt * 32;
                if (a.masked) {
                    const bf16x8_t t = *reinterpret_cast<const bf16x8_t*>(mrec + (dead ? 0 : nt * 32 + (gq >> 1) * 16));
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] *= ((float)t[i] > 0.f ? 1.f : a.slope);
                }
                bf16x8_t ov;
#pragma unroll
                for (int i = 0; i < 8; ++i) ov[i] = (__bf16)v[i];
                const u32x4_t ou = __builtin_bit_cast(u32x4_t, ov);
                if (LAST_PARTIAL && nt == NT - 1 && a.ypx != CXP * 2) __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{ou[0], ou[1]}, rs_y, off, 0, 0);      // dense: channels 16-19 only
                else __builtin_amdgcn_raw_buffer_store_b128(ou, rs_y, off, 0, 0);
            }
        }
        // ---- weight gradients of this tile: two k-steps of 4 x 8 centre pixels ----
#pragma unroll
        for (int ks = 0; ks < 8 / KROWS; ++ks) {
            const char* z0 = ldsZ + zb + ks * (KROWS * CW * PIXZ);
            const char* x0 = ldsX + xb + ks * (2 * KROWS * XW * PIXB);
            bf16x8_t bf[NTZ], bf2[NTZ];
#pragma unroll
            for (int nt = 0; nt < NTZ; ++nt) bf[nt] = mil_tr_pair(z0 + nt * 32, z0 + 4 * PIXZ + nt * 32);
            if (proj_i >= 0) {                   // wave-uniform
#pragma unroll
                for (int nt = 0; nt < NTZ; ++nt) bf2[nt] = mil_tr_pair(z0 + a.lds_z2_off + nt * 32, z0 + a.lds_z2_off + 4 * PIXZ + nt * 32);
            }
#pragma unroll
            for (int i = 0; i < MW; ++i) {
                if (wave + NW * i < MT) {         // wave-uniform
                    const bf16x8_t af = mil_tr_pair(x0 + woff[i], x0 + 8 * PIXB + woff[i]);
#pragma unroll
                    for (int nt = 0; nt < NTZ; ++nt)
                        wacc[i][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[nt], wacc[i][nt], 0, 0, 0);
                    if (i == proj_i) {
#pragma unroll
                        for (int nt = 0; nt < NTZ; ++nt)
                            waccp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf2[nt], waccp[nt], 0, 0, 0);
                    }
                }
            }
            if (bias_wave) {
#pragma unroll
                for (int nt = 0; nt < NTZ; ++nt)
                    waccb[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bf[nt], waccb[nt], 0, 0, 0);
            }
        }
    }

    // one slab per workgroup, the layout of wgrad_kernel<.., PROJ>: row = tap*CXP + ci, col = co; bias sums in row tile MT,
    // the projection's rows behind it
    constexpr int SLAB_COLS = NTZ * 16;
    constexpr size_t SLAB_ELEMS = (size_t)(MT + 1 + PMN) * 16 * SLAB_COLS;
    float* slab = a.slab + (size_t)blockIdx.x * SLAB_ELEMS;
    if (proj_i >= 0) {
#pragma unroll
        for (int nt = 0; nt < NTZ; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                slab[(size_t)((MT + 1 + proj_mt - PM0) * 16 + gq * 4 + e) * SLAB_COLS + nt * 16 + r] = waccp[nt][e];
    }
#pragma unroll
    for (int i = 0; i < MW; ++i) {
        const int mt = wave + NW * i;
        if (mt >= MT) continue;
#pragma unroll
        for (int nt = 0; nt < NTZ; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                slab[(size_t)(mt * 16 + gq * 4 + e) * SLAB_COLS + nt * 16 + r] = wacc[i][nt][e];
    }
    if (bias_wave) {
#pragma unroll
        for (int nt = 0; nt < NTZ; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                slab[(size_t)(MT * 16 + gq * 4 + e) * SLAB_COLS + nt * 16 + r] = waccb[nt][e];
    }
}

// MIL_ENTRY_BWD=0 (a test knob, read per call): never; unset or 1: wherever the kernel exists (its launch measured shorter
// than the two it replaces: DESIGN.md section 3.38).
static bool mil_entry_bwd_wanted() {
    const char* e = mil_test_knob("MIL_ENTRY_BWD");
    return !(e && e[0] == '0');
}

extern "C" int mil_conv_wgrad_pair_workspace(size_t* bytes, int n_img, int H, int W, int cin, int Ho, int Wo, int cout, int dtype);

template <int CZ, int NT, int NW>
static int run_entry_bwd(EntryBwdArgs a, float* dw3, float* db3, float* dw1, void* ws, size_t ws_bytes, int cout, int cin,
                         int accumulate, bool query, size_t* need, hipStream_t st) {
    constexpr int CXP = mil_nt_to_cp(NT), CGX = CXP / 8, PIXZ = mil_pix_pitch(CZ, 2), PIXB = mil_pix_pitch(CXP, 2);
    constexpr int MT = (9 * CGX + 1) / 2, NTZ = (CZ + 15) / 16, PMN = (5 * CGX - 1) / 2 - 2 * CGX + 1;
    // the pair kernel's tiles: 8x8 dz pixels (40 -> 60), or 16x8 (20 -> 40, dz maps with a side above 8) — one image each
    if (a.g.Ho <= 8 && a.g.Wo <= 8) return MIL_ERR_UNSUPPORTED;
    if (NW == 8 && a.g.H <= 8 && a.g.W <= 8) return MIL_ERR_UNSUPPORTED;
    mil_geom_set(a.g, NW == 8 ? 5 : 4, 4, 0);
    const size_t z_all = (size_t)a.g.n_img * a.g.H * a.g.W * CZ * 2, x_all = (size_t)a.g.n_img * a.g.Ho * a.g.Wo * CXP * 2;
    if (z_all > mil_buffer_limit() || x_all > mil_buffer_limit()) return MIL_ERR_UNSUPPORTED;     // one buffer descriptor per tensor
    const size_t y_all = (size_t)a.g.n_img * a.g.Ho * a.g.Wo * a.ypx;
    const int z_bytes = (9 * (NW == 8 ? 17 : 9) * PIXZ + 15) & ~15;
    const int w_bytes = mil_s2_nsteps(CZ / 8) * NT * 64 * 16;
    a.lds_z2_off = z_bytes; a.lds_w_off = 2 * z_bytes; a.lds_x_off = 2 * z_bytes + w_bytes;
    const int lds = a.lds_x_off + ((17 * (NW == 8 ? 33 : 17) * PIXB + 15) & ~15);
    if (lds > 160 * 1024) return MIL_ERR_UNSUPPORTED;
    auto kern = conv_entry_bwd_kernel<CZ, NT, NW>;
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return MIL_ERR_LAUNCH;
    const int ntiles = a.g.n_groups * a.g.tiles_y * a.g.tiles_x;
    const size_t slab_elems = (size_t)(MT + 1 + PMN) * 16 * NTZ * 16;
    // one slab per workgroup, and exactly the workgroups of the pair kernel (its resident set, at most one per tile): the same
    // tiles then meet in the same slab in the same order, and the reduction sums the same number of slabs
    size_t pair_bytes = 0;
    const int rc = mil_conv_wgrad_pair_workspace(&pair_bytes, a.g.n_img, a.g.Ho, a.g.Wo, cin, a.g.H, a.g.W, cout, MIL_DT_BF16);
    if (rc != MIL_OK) return rc;
    int grid = (int)(pair_bytes / (slab_elems * sizeof(float)));
    if (grid < 1 || grid > ntiles || (size_t)grid * slab_elems * sizeof(float) != pair_bytes) return MIL_ERR_UNSUPPORTED;
    if (mil_resident_per_cu(kern, lds, 2, 64 * NW) * mil_num_cus() < grid) return MIL_ERR_UNSUPPORTED;      // a second round would only add time
    {   // MIL_RES_GRID_CAP (test knob): fewer workgroups than tiles, so that a workgroup's accumulators carry across tiles
        const char* e = mil_test_knob("MIL_RES_GRID_CAP");
        const int cap = e ? atoi(e) : 0;
        if (cap > 0 && grid > cap) grid = cap;
    }
    const size_t bytes = slab_elems * grid * sizeof(float);
    if (query) { *need = bytes; return MIL_OK; }
    if (!ws || ws_bytes < bytes) return MIL_ERR_ARG;
    a.slab = (float*)ws;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, st, a, ntiles, (unsigned)z_all, (unsigned)x_all, (unsigned)y_all);
    MIL_CHECK_LAUNCH();
    MilReduceJob j{};
    j.slab = (const float*)ws; j.nslab = grid; j.slab_elems = slab_elems; j.slab_cols = NTZ * 16; j.n_rows = 9 * CXP;
    j.dw = dw3; j.db = db3; j.cout = cout; j.cin = cin; j.ks = 3; j.kind = 0; j.cinp = CXP; j.stem_mode = 0;
    j.bias_row = MT * 16; j.accumulate = accumulate;
    mil_reduce_or_defer(j, st);
    MIL_CHECK_LAUNCH();
    MilReduceJob j1 = j;                         // the projection's rows sit behind the bias tile: rows = input channel, one tap
    j1.slab = (const float*)ws + (size_t)(MT + 1) * 16 * NTZ * 16;
    j1.n_rows = CXP; j1.dw = dw1; j1.db = nullptr; j1.ks = 1; j1.bias_row = 0;
    mil_reduce_or_defer(j1, st);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

static int entry_bwd_entry(const void* dz1, const void* dz2, const void* wpack, const void* xin, void* dx, float* dw3, float* db3,
                           float* dw1, void* ws, size_t ws_bytes, int n_img, int h, int w, int cout, int H, int W, int cin,
                           int masked, float slope, int accumulate, int dtype, bool query, size_t* need, void* stream) {
    if (n_img < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return MIL_ERR_ARG;
    if ((dtype != MIL_DT_BF16 && dtype != MIL_DT_BF16_DGRAD) || n_img == 0 || h != (H - 1) / 2 + 1 || w != (W - 1) / 2 + 1 ||
        slope < 0.f || slope >= 1.f) return MIL_ERR_UNSUPPORTED;
    const int cz_p = mil_cpad(cout), cx_p = mil_cpad(cin);
    EntryBwdArgs a{};
    a.dz1 = (const __bf16*)dz1; a.dz2 = (const __bf16*)dz2; a.w = (const __bf16*)wpack; a.x = (const __bf16*)xin; a.y = (__bf16*)dx;
    a.g.n_img = n_img; a.g.H = h; a.g.W = w; a.g.Ho = H; a.g.Wo = W; a.g.ks = 3; a.g.stride = 1; a.g.pad = 1; a.g.zins = 1;
    a.slope = slope; a.masked = masked; a.ypx = cx_p * 2;
    if (dtype == MIL_DT_BF16_DGRAD) {            // dx [n,H,W,20] dense: the 40 -> 20 channel entry only
        if (cz_p != 40 || cx_p != 24) return MIL_ERR_UNSUPPORTED;
        a.ypx = 40;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the 20 -> 40 and 40 -> 60 channel entries; 60 -> 80 (its tiles do not fit LDS) keeps its launches: DESIGN.md section 3.38
    if (cz_p == 40 && cx_p == 24 && mil_entry_bwd_wanted())
        return run_entry_bwd<40, 2, 8>(a, dw3, db3, dw1, ws, ws_bytes, cout, cin, accumulate, query, need, st);
    if (cz_p == 64 && cx_p == 40 && mil_entry_bwd_wanted())
        return run_entry_bwd<64, 3, 4>(a, dw3, db3, dw1, ws, ws_bytes, cout, cin, accumulate, query, need, st);
    return MIL_ERR_UNSUPPORTED;
}

extern "C" int mil_conv_entry_bwd_workspace(size_t* bytes, int n_img, int h, int w, int cout, int H, int W, int cin, int dtype) {
    if (!bytes) return MIL_ERR_ARG;
    return entry_bwd_entry(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, n_img, h, w, cout, H, W,
                           cin, 0, 0.f, 0, dtype, true, bytes, nullptr);
}

// dx [n,H,W,cpad(cin)] = lrelu'(xin) * ( conv3x3_s2^T(dz1) + conv1x1_s2^T(dz2) ) exactly as mil_conv_dgrad_s2 computes it
// (masked = 0: no mask), AND dw3 [cout,cin,3,3], db3 [cout], dw1 [cout,cin,1,1] exactly as mil_conv_wgrad_pair computes them,
// from one pass (MIL_DT_BF16_DGRAD: dx [n,H,W,20]).  bf16; 40 -> 60 channels on maps above 8 pixels, 20 -> 40 above 16.
extern "C" int mil_conv_entry_bwd(const void* dz1, const void* dz2, const void* wpack, const void* xin, void* dx, float* dw3,
                                  float* db3, float* dw1, void* workspace, size_t workspace_bytes, int n_img, int h, int w,
                                  int cout, int H, int W, int cin, int masked, float slope, int accumulate, int dtype,
                                  void* stream) {
    if (!dz1 || !dz2 || !wpack || !xin || !dx || !dw3 || !db3 || !dw1 || !workspace) return MIL_ERR_ARG;
    size_t need = 0;
    return entry_bwd_entry(dz1, dz2, wpack, xin, dx, dw3, db3, dw1, workspace, workspace_bytes, n_img, h, w, cout, H, W, cin,
                           masked, slope, accumulate, dtype, false, &need, stream);
}
