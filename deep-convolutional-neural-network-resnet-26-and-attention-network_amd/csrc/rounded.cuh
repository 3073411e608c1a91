// Single correctly rounded operations that a neighbouring product or sum may not fuse with: what the kernels use whose
// outputs are held bit for bit to torch's or numpy's arithmetic on the CPU (path_attr.hip, feature_vis.hip, attr_render.hip).
// HIP's own __fmul_rn / __fadd_rn will not do: they are plain operators compiled with contraction allowed, so a product
// feeding a sum becomes one v_fma_f32.  These carry no `contract` flag.
#pragma once

#define MIL_ROUNDED_OP(name, type, op)                          \
    __device__ __forceinline__ type name(type a, type b) {      \
        _Pragma("clang fp contract(off)")                       \
        return a op b;                                          \
    }
MIL_ROUNDED_OP(rn_add, float, +)
MIL_ROUNDED_OP(rn_sub, float, -)
MIL_ROUNDED_OP(rn_mul, float, *)
MIL_ROUNDED_OP(rn_div, float, /)
MIL_ROUNDED_OP(rn_dadd, double, +)
MIL_ROUNDED_OP(rn_dsub, double, -)
MIL_ROUNDED_OP(rn_dmul, double, *)
MIL_ROUNDED_OP(rn_ddiv, double, /)
#undef MIL_ROUNDED_OP

// The correctly rounded square root: llvm.sqrt.f32, which hipcc lowers to the refined sequence unless it is told otherwise
// (-fhip-fp32-correctly-rounded-divide-sqrt, its default; the Makefile passes no fast-math flag).  HIP's own __fsqrt_rn is
// __ocml_native_sqrt_f32 in this toolchain — the bare v_sqrt_f32, one ulp — and does not give numpy's bits.
__device__ __forceinline__ float rn_sqrt(float a) { return __builtin_sqrtf(a); }
