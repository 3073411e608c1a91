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
#include "reduce.cuh"

// ---- the data gradient itself: shared by conv_dgrad_s2_kernel and conv_entry_bwd_kernel ------------------------------
// The second kernel's dx has to be the first one's bit for bit, so the tile fetch, the tap
// offsets, the MFMA loop and the store exist once, here; a kernel adds its tile walk and where its mask comes from.

// The two compact dz tiles of an output tile: per image ch x cw pixels of CZ channels, (1 << ti_log2) images, the same
// 16-byte pieces of both sources.  MULTI: a tile may hold several images (else ti_log2 is 0 and nothing is spent on the
// image index); extents a caller knows at compile time fold when passed as constants.
template <typename T, int CZ, int NP, int NTHR, bool MULTI>
struct S2ZTiles {
    static constexpr int ESZ = T::ESZ, N16 = CZ * ESZ / 16, PIXZ = mil_pix_pitch(CZ, ESZ), JB = T::SPLIT ? 8 : 16;
    HaloTables<NP> t;           // pos = (ti<<20)|(cy<<10)|cx or -1, lds / rel = byte offset in the LDS tile / from the tile's first dz pixel
    __device__ __forceinline__ void build(int tid, int ch, int cw, int ti_log2, int h, int w) {
        const int total = ((ch * cw) << ti_log2) * N16;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + NTHR * i;
            t.pos[i] = -1; t.lds[i] = 0; t.rel[i] = 0;
            if (idx < total) {
                const int p = idx / N16, j = idx - p * N16;
                const int cx = p % cw, row = p / cw, cy = MULTI ? row % ch : row, ti = MULTI ? row / ch : 0;
                t.pos[i] = (ti << 20) | (cy << 10) | cx;
                t.lds[i] = p * PIXZ + j * JB;
                t.rel[i] = ((ti * h + cy) * w + cx) * (CZ * ESZ) + j * 16;
            }
        }
    }
    // issue the loads of output tile `o` (zeros beyond the dz map and the launch's images)
    __device__ __forceinline__ void fetch(u32x4_t (&r1)[NP], u32x4_t (&r2)[NP], __amdgpu_buffer_rsrc_t rs_z1, __amdgpu_buffer_rsrc_t rs_z2,
                                          const TileOrigin& o, int h, int w, int n_img) const {
        const int i0 = o.oy0 >> 1, j0 = o.ox0 >> 1;
        const int base = ((o.img0 * h + i0) * w + j0) * (CZ * ESZ);
        const int ylim = h - i0, xlim = w - j0, ilim = n_img - o.img0;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = t.pos[i];
            const bool ok = p >= 0 && (!MULTI || (p >> 20) < ilim) && (MULTI ? (p >> 10) & 1023 : p >> 10) < ylim && (p & 1023) < xlim;
            const unsigned off = ok ? (unsigned)(base + t.rel[i]) : MIL_OOB;
            r1[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_z1, off, 0, 0);
            r2[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_z2, off, 0, 0);
        }
    }
    __device__ __forceinline__ void commit(char* ldsZ, int z2_off, const u32x4_t (&r1)[NP], const u32x4_t (&r2)[NP]) const {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (t.pos[i] >= 0) {
                mil_commit_piece<T, CZ * 2>(ldsZ + t.lds[i], r1[i]);
                mil_commit_piece<T, CZ * 2>(ldsZ + z2_off + t.lds[i], r2[i]);
            }
        }
    }
};

// toff[s]: where lane group gq reads its K-group of k-step s (the steps of the four parity classes in one sequence),
// relative to the class pixel's record in the first compact tile (rows of cw pixels, the second tile z2_off behind)
template <int CG, int PIXZ>
__device__ __forceinline__ void mil_s2_tap_offsets(int (&toff)[mil_s2_nsteps(CG)], int gq, int cw, int z2_off) {
    int s = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int sl = 0; sl < mil_s2_steps(c, CG); ++sl, ++s) {
            const S2Group gr = mil_s2_group(c, 4 * sl + gq, CG);
            toff[s] = gr.valid ? gr.src * z2_off + (gr.di * cw + gr.dj) * PIXZ + gr.cg * 16 : 0;
        }
    }
}

// Filter fragment (k-step st, column tile nt) of the MIL_PACK_DGRAD_S2 order: staged in LDS, or (split precision) streamed
// from L1/L2 — [hi | lo] = two 16-byte loads per lane, the fragment index in the scalar offset of the buffer load.
template <typename T, int NT>
struct S2FilterLds {
    const char* w; int lane;
    __device__ __forceinline__ Frag8<T> operator()(int st, int nt) const { return lds_frag<T>(w + ((st * NT + nt) * 64 + lane) * (8 * T::ESZ)); }
};
template <int NT>
struct S2FilterStream {
    __amdgpu_buffer_rsrc_t rs; int lane;
    __device__ __forceinline__ Frag8<F32S> operator()(int st, int nt) const {
        constexpr int FRAGB = 8 * F32S::ESZ;
        Frag8<F32S> f;
        f.h = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(lane * FRAGB), (st * NT + nt) * 64 * FRAGB, 0));
        f.l = __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(lane * FRAGB + 16), (st * NT + nt) * 64 * FRAGB, 0));
        return f;
    }
};

// acc[class][nt] = D[channel][pixel] of the four parity classes of the lane's class pixel (record at zpix).  One k-step
// ahead (the steps of the four classes flattened into one sequence): the fragments of step s+1 are read before the MFMAs
// of step s and scheduling fences keep that order (see mil_conv_ring); a streamed filter of fewer than four column tiles
// runs two k-steps ahead (8 VGPRs per split fragment).
template <typename T, int CZ, int NT, bool STREAM, class WFrag>
__device__ __forceinline__ void mil_s2_class_mma(f32x4_t (&acc)[4][NT], const char* zpix, const int (&toff)[mil_s2_nsteps(CZ / 8)], WFrag wfrag) {
    constexpr int CG = CZ / 8, NS = mil_s2_nsteps(CG);
    constexpr int WD = (STREAM && NT < 4) ? 2 : 1, WR = WD + 1;      // filter fragments in flight: k-steps ahead / ring slots
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[c][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto cls = [](int st) { int c = 0; while (st >= mil_s2_steps(c, CG)) { st -= mil_s2_steps(c, CG); ++c; } return c; };
    Frag8<T> xq[2], wq[WR][NT];
    xq[0] = lds_pix_frag<T, CZ * 2>(zpix + toff[0]);
#pragma unroll
    for (int k = 0; k < WD && k < NS; ++k)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wq[k % WR][nt] = wfrag(k, nt);
#pragma unroll
    for (int st = 0; st < NS; ++st) {
        if (st + 1 < NS) xq[(st + 1) & 1] = lds_pix_frag<T, CZ * 2>(zpix + toff[st + 1 < NS ? st + 1 : st]);
        if (st + WD < NS) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wq[(st + WD) % WR][nt] = wfrag(st + WD, nt);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[cls(st)][nt] = mma8(wq[st % WR][nt], xq[st & 1], acc[cls(st)][nt]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Epilogue: after one v_permlane16_swap per accumulator register between classes 2p (c0) and 2p+1 (c1) a lane holds 8
// consecutive channels (16*nt + 8*(gq>>1) ...) of output pixel (2i + p, 2j + (gq&1)).
__device__ __forceinline__ void mil_s2_pair8(const f32x4_t& c0, const f32x4_t& c1, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float lo = c0[i], hi = c1[i];
        if (i == 0) mil_swap16<true>(lo, hi); else mil_swap16<false>(lo, hi);
        v[i] = lo;
        v[4 + i] = hi;
    }
}
// ... and the bf16 store of that pixel's NT column tiles at byte offset ooff (+ 32 per column tile; MIL_OOB: none):
// times lrelu' of mask(nt, dead) — the block input's 8 channels there — when `masked`.  A record of 24 channels ends in the
// last tile's first half: lanes of the other half (`dead`) store nothing, and the dense 20-channel layout (ypx = 40) keeps
// channels 16-19 only.
template <int NT, class Mask>
__device__ __forceinline__ void mil_s2_store_bf16(const f32x4_t (&c0)[NT], const f32x4_t (&c1)[NT], __amdgpu_buffer_rsrc_t rs_y, unsigned ooff,
                                                  int gq, int ypx, bool masked, float slope, Mask mask) {
    constexpr int CXP = mil_nt_to_cp(NT);
    constexpr bool LAST_PARTIAL = (CXP % 16) != 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float v[8];
        mil_s2_pair8(c0[nt], c1[nt], v);
        const bool dead = LAST_PARTIAL && nt == NT - 1 && (gq >> 1) != 0;
        const unsigned off = dead ? MIL_OOB : ooff + nt * 32;
        if (masked) {
            const bf16x8_t t = mask(nt, dead);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] *= ((float)t[i] > 0.f ? 1.f : slope);
        }
        bf16x8_t ov;
#pragma unroll
        for (int i = 0; i < 8; ++i) ov[i] = (__bf16)v[i];
        const u32x4_t ou = __builtin_bit_cast(u32x4_t, ov);
        if (LAST_PARTIAL && nt == NT - 1 && ypx != CXP * 2) __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{ou[0], ou[1]}, rs_y, off, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b128(ou, rs_y, off, 0, 0);
    }
}

// Host side of both entry points: the argument rules, the geometry (output tiling: Ho=H, Wo=W (dx), H=h, W=w (dz)) and the
// bytes per pixel of dx — padded, or 20 dense channels (MIL_DT_BF16_DGRAD / MIL_DT_F32S_DGRAD: the 40 -> 20 channel entry only).
static int mil_s2_bwd_geom(ConvGeom& g, int& ypx, int n_img, int h, int w, int cz_p, int H, int W, int cx_p, float slope, int dtype) {
    if (n_img < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return MIL_ERR_ARG;
    const bool split = dtype == MIL_DT_F32S || dtype == MIL_DT_F32S_DGRAD, dense = dtype == MIL_DT_BF16_DGRAD || dtype == MIL_DT_F32S_DGRAD;
    if ((!split && dtype != MIL_DT_BF16 && dtype != MIL_DT_BF16_DGRAD) || h != (H - 1) / 2 + 1 || w != (W - 1) / 2 + 1 || slope < 0.f || slope >= 1.f)
        return MIL_ERR_UNSUPPORTED;
    if (n_img > 0 && dense && (cz_p != 40 || cx_p != 24)) return MIL_ERR_UNSUPPORTED;      // (an empty launch is the caller's to answer)
    g.n_img = n_img; g.H = h; g.W = w; g.Ho = H; g.Wo = W; g.ks = 3; g.stride = 1; g.pad = 1; g.zins = 1;
    ypx = (dense ? 20 : cx_p) * (split ? 4 : 2);
    return MIL_OK;
}

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
    S2ZTiles<T, CZ, NPZ, NTHR, true> zt;
    zt.build(tid, CH, CW, g.ti_log2, h, w);
    // class pixel of this lane: index wave*16 + r of the 64 (ti, i, j) positions; the same for all four classes
    const int cp = wave * 16 + r;
    const int cj = cp & (TW / 2 - 1), ci = (cp >> (g.tw_log2 - 1)) & (TH / 2 - 1), cti = cp >> (g.tw_log2 + g.th_log2 - 2);
    const int pixbase = ((cti * CH + ci) * CW + cj) * PIXZ;
    int toff[NS];
    mil_s2_tap_offsets<CG, PIXZ>(toff, gq, CW, a.lds_z2_off);
    // epilogue (mil_s2_pair8): output pixels (2i + p, 2j + (gq&1)), p = 0, 1
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
        zt.fetch(rz1, rz2, rs_z1, rs_z2, cur.origin(g), h, w, g.n_img);
        fetch_epi(cur.origin(g), ooff_n, ract_n);
    }
    const int G = gridDim.x;
    for (int tile = bid; tile < ntiles; tile += G) {
        const TileOrigin o_cur = cur.origin(g);
        __syncthreads();                       // every wave has finished reading the compact tiles of the previous tile
        if constexpr (NOPF) zt.fetch(rz1, rz2, rs_z1, rs_z2, o_cur, h, w, g.n_img);
        zt.commit(ldsZ, a.lds_z2_off, rz1, rz2);
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
            zt.fetch(rz1, rz2, rs_z1, rs_z2, nxt.origin(g), h, w, g.n_img);
            fetch_epi(nxt.origin(g), ooff_n, ract_n);
        }
        }
        cur = nxt; nxt.advance();

        f32x4_t acc[4][NT];
        if constexpr (STREAM) mil_s2_class_mma<T, CZ, NT, true>(acc, ldsZ + pixbase, toff, S2FilterStream<NT>{rs_w, lane});
        else mil_s2_class_mma<T, CZ, NT, false>(acc, ldsZ + pixbase, toff, S2FilterLds<T, NT>{ldsW, lane});
        if constexpr (NOPF) fetch_epi(o_cur, ooff, ract);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if constexpr (T::SPLIT) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    float v[8];
                    mil_s2_pair8(acc[2 * p][nt], acc[2 * p + 1][nt], v);
                    const unsigned off = (LAST_PARTIAL && nt == NT - 1 && !last_ok) ? MIL_OOB : ooff[p] + nt * 16 * ESZ;
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
                }
            } else {
                mil_s2_store_bf16<NT>(acc[2 * p], acc[2 * p + 1], rs_y, ooff[p], gq, a.ypx, a.act != nullptr, a.slope,
                                      [&](int nt, bool) { return __builtin_bit_cast(bf16x8_t, ract[p][nt][0]); });
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
    if (!dz1 || !wpack || !y) return MIL_ERR_ARG;
    ConvGeom g{};
    int ypx = 0;
    const int rc = mil_s2_bwd_geom(g, ypx, n_img, h, w, cz_p, H, W, cx_p, slope, dtype);
    if (rc != MIL_OK) return rc;
    if (n_img == 0) return MIL_OK;
    if (!((cz_p == 40 && cx_p == 24) || (cz_p == 64 && cx_p == 40) || (cz_p == 80 && cx_p == 64))) return MIL_ERR_UNSUPPORTED;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MIL_DT_F32S || dtype == MIL_DT_F32S_DGRAD) {      // fp32 tensors, bf16x3 products: all three entries, the filter streamed
        // (80 -> 64 channels: 64 accumulator + 64 fragment registers beside 25 per-lane tap offsets spill 58 VGPRs at two waves per
        // SIMD, so that entry runs ONE wave per SIMD with the next tile prefetched in registers — against 0.34 ms on the
        // zero-insert form of the generic kernel)
        DgradS2Args<F32S> b{};
        b.dz1 = (const float*)dz1; b.dz2 = (const float*)dz2; b.w = (const float*)wpack; b.act = (const float*)act; b.y = (float*)y;
        b.g = g; b.slope = slope; b.ypx = ypx;
        if (cz_p == 40) {               // staged filter: 0.52 ms against 0.60 ms streamed; eight waves on one staged filter where the map allows
            if (H >= 16 && W >= 32) return launch_dgrad_s2<F32S, 40, 2, false, 8>(b, st);
            return launch_dgrad_s2<F32S, 40, 2>(b, st);
        }
        if (cz_p == 64) return launch_dgrad_s2<F32S, 64, 3, true>(b, st);
        return launch_dgrad_s2<F32S, 80, 4, true>(b, st);
    }
    DgradS2Args<BF16> a{};
    a.dz1 = (const __bf16*)dz1; a.dz2 = (const __bf16*)dz2; a.w = (const __bf16*)wpack; a.act = (const __bf16*)act; a.y = (__bf16*)y;
    a.g = g; a.slope = slope; a.ypx = ypx;
    if (cz_p == 40) return launch_dgrad_s2<BF16, 40, 2>(a, st);
    if (cz_p == 64) return launch_dgrad_s2<BF16, 64, 3>(a, st);
    return launch_dgrad_s2<BF16, 80, 4>(a, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// Stage-entry backward in ONE launch (bf16): the data gradient above plus the weight gradients of the block's 3x3/s2 conv
// and 1x1/s2 projection and the conv's bias gradient — what wgrad_kernel<.., PROJ> computes in a second pass over the same
// three tensors.  Everything that pass reads is on chip here but the one-pixel top/left ring of the block input: the input
// is therefore staged as a tile of [pixel][channel] records, one row and one column more than the output tile (record
// (ry,rx) = input pixel (oy0 - 1 + ry, ox0 - 1 + rx), zero outside the image), the mask is read back from that tile, and
// per tile the 32-pixel k-steps over the CENTRE pixels of the compact dz tiles (the halo row and column belong to the
// neighbouring tiles) feed
//     dW1[(tap,ci)][co] += sum_q x[2q + tap - 1][ci] * dz1[q][co],   dWp[ci][co] += sum_q x[2q][ci] * dz2[q][co],
//     db1[co] += sum_q dz1[q][co]
// with both operands read by ds_read_b64_tr_b16 (per-lane addresses: the stride-2 gather of x costs nothing extra).  The
// accumulators stay in registers over the workgroup's whole tile walk; at the end every workgroup writes ONE MilWgradSlab.
// The weight gradients are mil_conv_wgrad_pair's BIT FOR BIT: on that launch's grid and dz tiles (mil_wgrad_pair_plan) this
// kernel walks the tiles in the same order, pixel p of a tile sits in the same k-step and the same MFMA k-slot in both, so
// every slab element is the same sequence of MFMAs.
// LDS: [dz1 9x9][dz2 9x9][filter][x 17x17] (NW = 8: 9x17, 17x33).
struct EntryBwdArgs {
    const __bf16* dz1;      // [n,h,w,CZ]
    const __bf16* dz2;      // [n,h,w,CZ]
    const __bf16* w;        // MIL_PACK_DGRAD_S2 fragments
    const __bf16* x;        // [n,H,W,CXP]  block input: weight-gradient operand and (masked) lrelu' mask
    __bf16* y;              // [n,H,W,CXP], or dense ([n,H,W,20], ypx = 40)
    float* slab;            // [gridDim.x] MilWgradSlab<3, CXP, NTZ, true>
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
template <int NW> struct EntryBwdTile { static constexpr int TW_LOG2 = NW == 8 ? 4 : 3, TH_LOG2 = 3; };      // in dz pixels, one image
template <int CZ, int NT, int NW>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void conv_entry_bwd_kernel(EntryBwdArgs a, int ntiles, unsigned z_bytes, unsigned x_bytes, unsigned y_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MIL_POISON(smem);
    using T = BF16;
    constexpr int CG = CZ / 8, N16 = CZ * 2 / 16, PIXZ = mil_pix_pitch(CZ, 2);
    constexpr int CXP = mil_nt_to_cp(NT), CGX = CXP / 8, X16 = CXP * 2 / 16, PIXB = mil_pix_pitch(CXP, 2);
    constexpr int NS = mil_s2_nsteps(CG);
    constexpr int ZW = 1 << EntryBwdTile<NW>::TW_LOG2, ZH = 1 << EntryBwdTile<NW>::TH_LOG2;
    constexpr int NTHR = 64 * NW, CH = ZH + 1, CW = ZW + 1, XH = 2 * ZH + 1, XW = 2 * ZW + 1;
    constexpr int NPZ = (CH * CW * N16 + NTHR - 1) / NTHR, NPX = (XH * XW * X16 + NTHR - 1) / NTHR;
    // weight-gradient GEMM: M = (tap, ci) in row groups of 8 channels, N = co, K = the tile's centre dz pixels
    constexpr int NTZ = (CZ + 15) / 16;
    using Slab = MilWgradSlab<3, CXP, NTZ, true>;
    constexpr int RG = Slab::RG, MT = Slab::MT, MW = (MT + NW - 1) / NW;
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
    S2ZTiles<T, CZ, NPZ, NTHR, false> zt;
    zt.build(tid, CH, CW, 0, h, w);
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
    // data gradient: class pixel of this lane, index wave*16 + r of the (i, j) positions, the same for all four classes
    const int cp = wave * 16 + r;
    const int cj = cp & (ZW - 1), ci = cp >> EntryBwdTile<NW>::TW_LOG2;
    const int pixbase = (ci * CW + cj) * PIXZ;
    int toff[NS];
    mil_s2_tap_offsets<CG, PIXZ>(toff, gq, CW, a.lds_z2_off);
    // weight gradient: lane (gq, q4, p4) reads 4 channels of pixel (row gq, column q4 / q4 + 4) of a k-step's 4 x 8 pixels
    const int q4 = r >> 2, p4 = r & 3;
    // (the pair kernel's pixel order: pixel 8*gq + q4 (+ 4) of a k-step's 32, row-major over a tile 8 or 16 pixels wide)
    const int krow = NW == 8 ? gq >> 1 : gq, kcol = (NW == 8 ? (gq & 1) * 8 : 0) + q4;
    const int zb = (krow * CW + kcol) * PIXZ + p4 * 8;
    const int xb = (2 * krow * XW + 2 * kcol) * PIXB + (p4 & 1) * 8;
    constexpr int KROWS = 32 / ZW;              // dz rows per k-step
    int woff[MW];
    int proj_i = -1, proj_mt = 0;               // the owned row tile (at most one per wave) that also feeds the projection
#pragma unroll
    for (int i = 0; i < MW; ++i) {
        const int mt = wave + NW * i;
        if (mt < MT && Slab::feeds_proj(mt)) { proj_i = i; proj_mt = mt; }
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
        zt.fetch(rz1, rz2, rs_z1, rs_z2, o, h, w, g.n_img);
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
        zt.commit(ldsZ, a.lds_z2_off, rz1, rz2);
#pragma unroll
        for (int i = 0; i < NPX; ++i)
            if (x_pos[i] >= 0) *reinterpret_cast<u32x4_t*>(ldsX + x_lds[i]) = rx[i];
        __syncthreads();
        if (tile + G < ntiles) fetch(nxt.origin(g));
        cur = nxt; nxt.advance();

        // ---- data gradient; the mask comes from the x tile ----
        f32x4_t acc[4][NT];
        mil_s2_class_mma<T, CZ, NT, false>(acc, ldsZ + pixbase, toff, S2FilterLds<T, NT>{ldsW, lane});
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int oy = 2 * ci + p, ox = 2 * cj + (gq & 1);
            const bool ok = oy < H - o_cur.oy0 && ox < W - o_cur.ox0;
            const unsigned ooff = ok ? (unsigned)((((o_cur.img0 * H + o_cur.oy0 + oy) * W + o_cur.ox0 + ox)) * a.ypx + (gq >> 1) * 16) : MIL_OOB;
            const char* mrec = ldsX + ((oy + 1) * XW + ox + 1) * PIXB;
            mil_s2_store_bf16<NT>(acc[2 * p], acc[2 * p + 1], rs_y, ooff, gq, a.ypx, a.masked != 0, a.slope,
                                  [&](int nt, bool dead) { return *reinterpret_cast<const bf16x8_t*>(mrec + (dead ? 0 : nt * 32 + (gq >> 1) * 16)); });
        }
        // ---- weight gradients of this tile: k-steps of 32 centre pixels ----
#pragma unroll
        for (int ks = 0; ks < ZH / KROWS; ++ks) {
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

    float* slab = a.slab + (size_t)blockIdx.x * Slab::ELEMS;
    if (proj_i >= 0) Slab::store(slab, Slab::proj_tile(proj_mt), waccp, lane);
#pragma unroll
    for (int i = 0; i < MW; ++i)
        if (wave + NW * i < MT) Slab::store(slab, wave + NW * i, wacc[i], lane);
    if (bias_wave) Slab::store(slab, Slab::BIAS_TILE, waccb, lane);
}

// MIL_ENTRY_BWD=0 (a test knob, read per call): never; unset or 1: wherever the kernel exists (its launch measured shorter
// than the two it replaces: DESIGN.md section 3.38).
static bool mil_entry_bwd_wanted() {
    const char* e = mil_test_knob("MIL_ENTRY_BWD");
    return !(e && e[0] == '0');
}

template <int CZ, int NT, int NW>
static int run_entry_bwd(EntryBwdArgs a, float* dw3, float* db3, float* dw1, void* ws, size_t ws_bytes, int cout, int cin,
                         int accumulate, bool query, size_t* need, hipStream_t st) {
    constexpr int CXP = mil_nt_to_cp(NT), PIXZ = mil_pix_pitch(CZ, 2), PIXB = mil_pix_pitch(CXP, 2);
    using Slab = MilWgradSlab<3, CXP, (CZ + 15) / 16, true>;
    using Tile = EntryBwdTile<NW>;
    // one slab per workgroup, and exactly the workgroups of the pair kernel (its resident set, at most one per tile) on its
    // dz tiles — 8x8 pixels of one image (40 -> 60), or 16x8 (20 -> 40, dz maps with a side above 8): the same tiles then
    // meet in the same slab in the same order, and the reduction sums the same number of slabs.  Where the pair kernel
    // would tile differently (smaller maps) this kernel has no form.
    MilWgradPairPlan plan{};
    const int rc = mil_wgrad_pair_plan(&plan, a.g.n_img, a.g.Ho, a.g.Wo, cin, a.g.H, a.g.W, cout);
    if (rc != MIL_OK) return rc;
    if (plan.tw_log2 != Tile::TW_LOG2 || plan.th_log2 != Tile::TH_LOG2 || plan.ti_log2 != 0) return MIL_ERR_UNSUPPORTED;
    mil_geom_set(a.g, Tile::TW_LOG2 + 1, Tile::TH_LOG2 + 1, 0);
    const size_t z_all = (size_t)a.g.n_img * a.g.H * a.g.W * CZ * 2, x_all = (size_t)a.g.n_img * a.g.Ho * a.g.Wo * CXP * 2;
    if (z_all > mil_buffer_limit() || x_all > mil_buffer_limit()) return MIL_ERR_UNSUPPORTED;     // one buffer descriptor per tensor
    const size_t y_all = (size_t)a.g.n_img * a.g.Ho * a.g.Wo * a.ypx;
    constexpr int ZW = 1 << Tile::TW_LOG2, ZH = 1 << Tile::TH_LOG2;
    const int z_bytes = ((ZH + 1) * (ZW + 1) * PIXZ + 15) & ~15;
    const int w_bytes = mil_s2_nsteps(CZ / 8) * NT * 64 * 16;
    a.lds_z2_off = z_bytes; a.lds_w_off = 2 * z_bytes; a.lds_x_off = 2 * z_bytes + w_bytes;
    const int lds = a.lds_x_off + (((2 * ZH + 1) * (2 * ZW + 1) * PIXB + 15) & ~15);
    if (lds > 160 * 1024) return MIL_ERR_UNSUPPORTED;
    auto kern = conv_entry_bwd_kernel<CZ, NT, NW>;
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return MIL_ERR_LAUNCH;
    const int ntiles = a.g.n_groups * a.g.tiles_y * a.g.tiles_x;
    int grid = plan.grid;
    if (grid < 1 || grid > ntiles) return MIL_ERR_UNSUPPORTED;
    if (mil_resident_per_cu(kern, lds, 2, 64 * NW) * mil_num_cus() < grid) return MIL_ERR_UNSUPPORTED;      // a second round would only add time
    {   // MIL_RES_GRID_CAP (test knob): fewer workgroups than tiles, so that a workgroup's accumulators carry across tiles
        const char* e = mil_test_knob("MIL_RES_GRID_CAP");
        const int cap = e ? atoi(e) : 0;
        if (cap > 0 && grid > cap) grid = cap;
    }
    const size_t bytes = Slab::ELEMS * grid * sizeof(float);
    if (query) { *need = bytes; return MIL_OK; }
    if (!ws || ws_bytes < bytes) return MIL_ERR_ARG;
    a.slab = (float*)ws;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, st, a, ntiles, (unsigned)z_all, (unsigned)x_all, (unsigned)y_all);
    MIL_CHECK_LAUNCH();
    return Slab::reduce((const float*)ws, grid, dw3, db3, dw1, cout, cin, 0, accumulate, st);
}

static int entry_bwd_entry(const void* dz1, const void* dz2, const void* wpack, const void* xin, void* dx, float* dw3, float* db3,
                           float* dw1, void* ws, size_t ws_bytes, int n_img, int h, int w, int cout, int H, int W, int cin,
                           int masked, float slope, int accumulate, int dtype, bool query, size_t* need, void* stream) {
    const int cz_p = mil_cpad(cout), cx_p = mil_cpad(cin);
    EntryBwdArgs a{};
    const int rc = mil_s2_bwd_geom(a.g, a.ypx, n_img, h, w, cz_p, H, W, cx_p, slope, dtype);
    if (rc != MIL_OK) return rc;
    if ((dtype != MIL_DT_BF16 && dtype != MIL_DT_BF16_DGRAD) || n_img == 0) return MIL_ERR_UNSUPPORTED;
    a.dz1 = (const __bf16*)dz1; a.dz2 = (const __bf16*)dz2; a.w = (const __bf16*)wpack; a.x = (const __bf16*)xin; a.y = (__bf16*)dx;
    a.slope = slope; a.masked = masked;
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
