// LDS stage images and the MFMA stage of the 64 x 64 x 32 gather contractions (cb_geomconv.hip, cb_tconv.hip): written
// once, included by both translation units.
#pragma once
#include "cb_common.h"

namespace {

typedef unsigned short ushortx8 __attribute__((ext_vector_type(8)));

#define CBG_ROW16 40      // LDS row of 32 16-bit k-slots + 16 bytes (16-byte fragment reads free of conflicts)
#define CBG_ROW32 33

// LDS image of one operand (64 rows x 32 k) per arithmetic, and how 8 consecutive k of a row get there
template <int ARITH>
struct CbgStage;
template <>
struct CbgStage<CB_F16> {
    cb_half v[64][CBG_ROW16];
    __device__ __forceinline__ void put(int row, int k0, const cb_half (&x)[8]) {
        halfx8 t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = x[i];
        *(halfx8*)&v[row][k0] = t;
    }
};
template <>
struct CbgStage<CB_F32S> {
    unsigned short v[3][64][CBG_ROW16];
    __device__ __forceinline__ void put(int row, int k0, const float (&x)[8]) {
        ushortx8 h, m, l;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            unsigned a, b, c;
            cb_split3(x[i], a, b, c);
            h[i] = (unsigned short)a, m[i] = (unsigned short)b, l[i] = (unsigned short)c;
        }
        *(ushortx8*)&v[0][row][k0] = h;
        *(ushortx8*)&v[1][row][k0] = m;
        *(ushortx8*)&v[2][row][k0] = l;
    }
};
template <>
struct CbgStage<CB_F32> {
    float v[64][CBG_ROW32];
    __device__ __forceinline__ void put(int row, int k0, const float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[row][k0 + i] = x[i];
    }
};

template <int ARITH>
__device__ __forceinline__ floatx16 cbg_mfma_stage(const CbgStage<ARITH>& A, const CbgStage<ARITH>& B, int ra, int rb,
                                                   int lane, floatx16 acc) {
    const int kg = lane >> 5;
    if constexpr (ARITH == CB_F16) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const halfx8 a = *(const halfx8*)&A.v[ra][s * 16 + kg * 8], b = *(const halfx8*)&B.v[rb][s * 16 + kg * 8];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
    } else if constexpr (ARITH == CB_F32S) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k0 = s * 16 + kg * 8;
            const bf16x8 ah = *(const bf16x8*)&A.v[0][ra][k0], am = *(const bf16x8*)&A.v[1][ra][k0],
                         al = *(const bf16x8*)&A.v[2][ra][k0];
            const bf16x8 bh = *(const bf16x8*)&B.v[0][rb][k0], bm = *(const bf16x8*)&B.v[1][rb][k0],
                         bl = *(const bf16x8*)&B.v[2][rb][k0];
            // the six cross products above 2^-24 of the product, smallest first
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A.v[ra][2 * s + kg], B.v[rb][2 * s + kg], acc, 0, 0, 0);
    }
    return acc;
}

}  // namespace
