// The uint8 tile feed: tiles as planar bytes u [T,3,H,W], standing for the fp32 tensor ToTensor + Normalize(.5,.5) makes of
// them (RoiBuilder.py:193-210): v = ((u / 255) - 0.5) / 0.5, one of 256 fp32 values.  Used by stem_fused.hip (tiled and
// row-walk forward), conv_wgrad.hip (tiled backward) and pointwise.hip (stem_s2d from bytes, the host copy of the values).
//
// The decode has to reproduce an IEEE division: u * (1/255.f) differs from u / 255.f for 126 of the 256 codes,
// (u * (1/255.f) - 0.5f) * 2 is wrong for 111 and fma(u, 2/255.f, -1) for 205.  mil_u8_decode takes the reciprocal product and
// ONE Newton correction step (two fmas), which gives RN(u / 255) for every code, then fma(t, 2, -1) = RN(t - 0.5) * 2 exactly:
// five vector instructions per element, no memory.  The same expression compiles for the host (mil_u8_decode_table), where
// tests/test_cpu_u8_feed.py holds all 256 values to torch's.  Measured against a 256-entry [hi | lo] table in LDS (one ds_read_b32
// per element, no convert and no split): forward equal within the spread, tiled backward 4-9 % faster this way (its commit sits
// between two barriers, where the table reads' latency and bank conflicts on random bytes are exposed) — DESIGN.md §3.u8.
//
// Padding: code 0 decodes to -1.0, not to 0.  A lane whose load lies outside the image (border, rows above / below, unused
// load slots) commits zeros — the conv's padding — by its `ok` flag, never decode(0).
#pragma once
#include <cstdint>
#include "pf_common.cuh"

__host__ __device__ __forceinline__ float mil_u8_decode(unsigned code) {
    const float u = (float)code, inv = 1.0f / 255.0f;
    float t = u * inv;
    t = __builtin_fmaf(__builtin_fmaf(-t, 255.0f, u), inv, t);      // Newton step: t = RN(u / 255) for all 256 codes
    return __builtin_fmaf(t, 2.0f, -1.0f);                          // = (t - 0.5) / 0.5
}

// One load item = four consecutive columns of one colour plane in two image rows: w0 = bytes of row 2r, w1 = row 2r+1.
// pa / pb = s2d channels 4c..4c+3 (dy*2 + dx) of the first / second s2d pixel (hi halves); qa / qb = lo halves (X3 only:
// mil_split4, as the fp32 feed splits).  !ok: zeros.
template <bool X3>
__device__ __forceinline__ void mil_u8_item(unsigned w0, unsigned w1, bool ok, bf16x4_t& pa, bf16x4_t& pb, bf16x4_t& qa, bf16x4_t& qb) {
    const f32x4_t fa{mil_u8_decode(w0 & 255u), mil_u8_decode((w0 >> 8) & 255u), mil_u8_decode(w1 & 255u), mil_u8_decode((w1 >> 8) & 255u)};
    const f32x4_t fb{mil_u8_decode((w0 >> 16) & 255u), mil_u8_decode(w0 >> 24), mil_u8_decode((w1 >> 16) & 255u), mil_u8_decode(w1 >> 24)};
    if constexpr (X3) {
        mil_split4(fa, pa, qa);
        mil_split4(fb, pb, qb);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { pa[j] = (__bf16)fa[j]; pb[j] = (__bf16)fb[j]; }
    }
    auto keep = [ok](bf16x4_t& v) {
        u32x2_t w = __builtin_bit_cast(u32x2_t, v);
        w[0] = ok ? w[0] : 0u; w[1] = ok ? w[1] : 0u;
        v = __builtin_bit_cast(bf16x4_t, w);
    };
    keep(pa); keep(pb);
    if constexpr (X3) { keep(qa); keep(qb); }
}
