// LDS stage images and the MFMA stage of the 64 x 64 x 32 gather contractions (cb_geomconv.hip, cb_tconv.hip), and the
// mask -> list prologue and list lookup of cb_geomconv.hip and cb_groupconv.hip: written once, included by the
// translation units that use them.
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

// ---------------------------------------------------------------------------------------------
// The change list of a mask-mode launch (cbg_conv_kernel, cbgr_conv_kernel; 256 threads): every workgroup counts the
// bits of the mask the parity selects -- thread t the words [t chunk, (t + 1) chunk), chunk = ceil(words / 256) -- and
// scans the 256 counts into sPre[257]; for its share of the words (w % gridDim.x == blockIdx.x) it writes the ascending
// list entries, the mask copy and the zeros of the OTHER mask (the next frame's); the last workgroup to arrive flips the
// parity.  Returns the number of listed pixels, `cur` the frame's mask.  sWave: four ints of LDS.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int cbg_list_from_mask(unsigned long long* frameMasks, long words, int chunk, int wpr, int Wo,
                                                  int32_t* listOut, int32_t* countOut, int* sPre, int* sWave,
                                                  const unsigned long long*& cur) {
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int G = gridDim.x;
    int* ctl = (int*)(frameMasks + 2 * words);
    const int par = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cur = frameMasks + (par ? words : 0);
    unsigned long long* other = frameMasks + (par ? 0 : words);
    unsigned long long* copy = frameMasks + 2 * words + 2;
    const long w0 = (long)t * chunk, w1 = min(words, w0 + chunk);
    int cnt = 0;
    for (long w = w0; w < w1; ++w) cnt += __popcll(cur[w]);
    // inclusive scan of the 256 chunk counts: within each wave by lane shifts, then the four wave totals
    int inc = cnt;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const int up = __shfl_up(inc, dlt, 64);
        if (lane >= dlt) inc += up;
    }
    if (lane == 63) sWave[wave] = inc;
    __syncthreads();
    for (int i = 0; i < wave; ++i) inc += sWave[i];
    sPre[t + 1] = inc;
    if (t == 0) sPre[0] = 0;
    __syncthreads();
    const int N = sPre[256];
    // every workgroup writes the list entries, the mask copy and the zeros of the OTHER mask (the next frame's) for
    // its share of the words
    int run = sPre[t];
    for (long w = w0; w < w1; ++w) {
        const unsigned long long mw = cur[w];
        if ((int)(w % G) == (int)blockIdx.x) {
            const int yy = (int)(w / wpr), xx = (int)(w % wpr) * 64;
            unsigned long long r = mw;
            int at = run;
            while (r) {
                listOut[at++] = yy * Wo + xx + __builtin_ctzll(r);
                r &= r - 1;
            }
            copy[w] = mw;
            other[w] = 0ull;
        }
        run += __popcll(mw);
    }
    if (blockIdx.x == 0 && t == 0) countOut[0] = N;
    // every workgroup has read the parity and the mask by now: the last one to arrive flips the parity
    __syncthreads();
    if (t == 0 && __hip_atomic_fetch_add(ctl + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) {
        __hip_atomic_store(ctl + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ctl, par ^ 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return N;
}

// Entry q of the list (q < N checked by the caller's tile): from the mask `cur` through the scan sPre -- the last thread
// chunk whose prefix is <= q, then the words of that chunk -- or from a caller's list; -1 for an entry outside the map
// (a foreign list is not trusted with addresses).
__device__ __forceinline__ int cbg_list_entry(int q, const unsigned long long* cur, const int* sPre, long words, int chunk,
                                              int wpr, int Wo, const int32_t* list, int HWo) {
    int pix = -1;
    if (cur) {
        int lo = 0, hi = 255;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (sPre[mid] <= q) lo = mid; else hi = mid - 1;
        }
        int r = q - sPre[lo];
        long w = (long)lo * chunk;
        const long wEnd = min(words, w + chunk);
        unsigned long long mw = 0ull;
        for (; w < wEnd; ++w) {
            mw = cur[w];
            const int c = __popcll(mw);
            if (r < c) break;
            r -= c;
        }
        if (w < wEnd) pix = (int)(w / wpr) * Wo + (int)(w % wpr) * 64 + cb_select_bit(mw, r);
    } else {
        pix = list[q];
    }
    if (pix < 0 || pix >= HWo) pix = -1;
    return pix;
}

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
