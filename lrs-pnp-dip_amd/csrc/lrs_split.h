// The fp32-accurate product on the bf16 matrix cores (gfx950), the one definition every split-bf16
// kernel is built from: the resident ISTA kernels (ista.hip), the dictionary-learning GEMM
// (dictlearn.hip) and the DIP engine's GEMMs and convs (dip_gemm.h, dip_sm.h).
//
// v_mfma_f32_16x16x32_bf16 runs at 16x the f32 MFMA rate and, unlike the f32 MFMA, not on the VALU's
// FMA datapath.  Every fp32 operand is split exactly into three bf16 terms, v = v0 + v1 + v2 (8
// significand bits each: 24 = fp32; the remainder after v2 is below 2^-24 relative); of the nine
// products A_i B_j the six with i + j <= 2 are kept (the dropped ones are <= 2^-24 relative) and
// accumulated in fp32, small terms first, so each product has fp32-GEMM accuracy (not the bitwise f32
// MFMA result; parity is held to the same 1e-5 relative L2 as the rest of the pipeline).
//
// A change of the split or of the chain order is an edit here alone.  The subsystems' 1e-5 parity tests
// cannot see it (a lost product costs 2.4e-6); tests/test_gpu_split_accuracy.py holds every launched
// product to 3 x a sequential fp32 GEMM's error against fp64, and tests/test_split_emu.py shows on the
// CPU that a degraded chain exceeds that bound.
#pragma once
#include "lrs_common.h"

namespace lrs {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// x == (float)b0 + (float)b1 + (float)b2 up to 2^-24 relative; each subtraction is exact
struct Bf16Split {
    __bf16 b0, b1, b2;
};
__device__ __forceinline__ Bf16Split split_bf16(float x) {
    Bf16Split r;
    r.b0 = (__bf16)x;
    const float r1 = x - (float)r.b0;
    r.b1 = (__bf16)r1;
    r.b2 = (__bf16)(r1 - (float)r.b1);
    return r;
}

// 8 consecutive floats -> plane p_i = the 8 terms b_i: one 16-B LDS write per plane.  (Three
// references, not an array: with bf16x8 p[3] the GEMM kernels compile to different code.)
__device__ __forceinline__ void split_bf16x8(const float *v, bf16x8 &p0, bf16x8 &p1, bf16x8 &p2) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const Bf16Split q = split_bf16(v[e]);
        p0[e] = q.b0;
        p1[e] = q.b1;
        p2[e] = q.b2;
    }
}

// acc += A B over 32 k with both operands split three ways (lane l supplies A[l & 15][8 (l >> 4) + 0..7]
// and B[8 (l >> 4) + 0..7][l & 15]; acc holds C[4 (l >> 4) + r][l & 15], cdna_hip_programming.md §3).
// Order: A_lo B_hi, A_mid B_mid, A_hi B_lo, A_mid B_hi, A_hi B_mid, A_hi B_hi -- smallest first, so the
// low-order terms are not absorbed by an accumulator that already holds the leading product.
__device__ __forceinline__ floatx4 split_mfma6(const bf16x8 (&A)[3], const bf16x8 (&B)[3], floatx4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[2], B[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[0], acc, 0, 0, 0);
    return acc;
}

}  // namespace lrs
