// Shared definitions for the gfx950 kernels of libcbinfer_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbinfer_hip.h"

#define CB_WAVE 64

typedef _Float16 cb_half;

// MFMA tile geometry of the contraction kernels (cb_conv.hip).  The prepared weight matrix is
// padded to these so the k-loop and the m-tiles need no bounds checks.
#define CB_MFMA_M 32      // out-channel rows per MFMA tile
#define CB_BK 16          // k-depth staged in LDS per step (fp32); fp16 uses 32
#define CB_BK_H 32

// MFMA operand / accumulator vectors and the constant address space (scalar loads), shared by every kernel file
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(4))) int cb_const_int;

static inline int cb_div_up(long a, long b) { return (int)((a + b - 1) / b); }

// CU count of the current device, asked once per process (256 if the runtime will not say)
inline int cb_num_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            cus = n;
        else
            cus = 256;
    }
    return cus;
}

static inline int cb_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CB_OK : (int)e;
}

#define CB_REQUIRE(cond)                 \
    do {                                 \
        if (!(cond)) return CB_ERR_BADARG; \
    } while (0)

template <typename T>
struct cb_traits;
template <>
struct cb_traits<float> {
    static constexpr int dtype = CB_F32;
};
template <>
struct cb_traits<cb_half> {
    static constexpr int dtype = CB_F16;
};

// change predicate, one channel value
//   fp32: fabs(state - in) > th                                  (cbconv2d_cg_backend.cu:22,56)
//   fp16: d = __hsub(state, in); d > th16 | d < -th16            (cbconv2d_cg_half_backend.cu:27-28)
// bit-for-bit inequality (a value that equals the state is not written again by the copy-all detections)
__device__ __forceinline__ bool cb_differs(float s, float x) {
    return __builtin_bit_cast(unsigned, s) != __builtin_bit_cast(unsigned, x);
}
__device__ __forceinline__ bool cb_differs(cb_half s, cb_half x) {
    return __builtin_bit_cast(unsigned short, s) != __builtin_bit_cast(unsigned short, x);
}
__device__ __forceinline__ bool cb_changed(float s, float x, float th) {
    return fabsf(s - x) > th;
}
__device__ __forceinline__ bool cb_changed(cb_half s, cb_half x, cb_half th) {
    cb_half d = s - x;  // v_sub_f16: one rounding, like __hsub
    return (d > th) | (d < -th);
}
// max pooling primitives (shared by the pool kernel and the pooled change detection)
__device__ __forceinline__ float cb_neg_inf(float*) { return -INFINITY; }
__device__ __forceinline__ cb_half cb_neg_inf(cb_half*) { return (cb_half)(-INFINITY); }
__device__ __forceinline__ float cb_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ cb_half cb_max(cb_half a, cb_half b) { return a < b ? b : a; }
__device__ __forceinline__ float cb_threshold(float th, float*) { return th; }
__device__ __forceinline__ cb_half cb_threshold(float th, cb_half*) { return (cb_half)th; }  // RNE

// r-th (0-based) set bit of w, r < popcount(w)
__device__ __forceinline__ int cb_select_bit(unsigned long long w, int r) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const unsigned long long lowmask = ((1ull << width) - 1ull) << pos;
        const int c = __popcll(w & lowmask);
        if (r >= c) {
            r -= c;
            pos += width;
        }
    }
    return pos;
}

// the bits of word `tile` of a row's change mask that are pixels of a W-wide image
__device__ __forceinline__ unsigned long long cb_valid_mask(int W, int tile) {
    const int rem = W - tile * 64;
    return rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
}

// Horizontal dilation by kWH pixels of word `tile` of a row's change mask (wpr words, W pixels): D the word's own bits,
// SR / SL what spills into the next / the previous word, all three cut to the pixels of the row.
struct cb_dilated {
    unsigned long long D, SR, SL;
};
__device__ __forceinline__ cb_dilated cb_dilate_word(unsigned long long m, int kWH, int W, int tile, int wpr) {
    cb_dilated r = {m, 0ull, 0ull};
    for (int d = 1; d <= kWH; ++d) {
        r.D |= (m << d) | (m >> d);
        r.SR |= m >> (64 - d);
        r.SL |= m << (64 - d);
    }
    r.D &= cb_valid_mask(W, tile);
    r.SR = (tile + 1 < wpr) ? (r.SR & cb_valid_mask(W, tile + 1)) : 0ull;
    if (tile == 0) r.SL = 0ull;
    return r;
}
// ... ORed by one wave into the rows y - kHH .. y + kHH of an H-row mask: lane = (row, word).  The three words BY VALUE:
// handed over as a reference to the struct, the compiler keeps them in LDS (or scratch) for the indexed read below.
__device__ __forceinline__ void cb_or_dilated_rows(unsigned long long* bits, unsigned long long D, unsigned long long SR,
                                                   unsigned long long SL, int y, int kHH, int H, int tile, int wpr,
                                                   int lane) {
    const int items = 3 * (2 * kHH + 1);
    for (int i = lane; i < items; i += 64) {
        const int yy = y + i / 3 - kHH;
        const int which = i % 3;
        if (yy < 0 || yy >= H) continue;
        const unsigned long long v = which == 0 ? D : (which == 1 ? SR : SL);
        const int t2 = which == 0 ? tile : (which == 1 ? tile + 1 : tile - 1);
        if (v) atomicOr(&bits[(long)yy * wpr + t2], v);
    }
}

// Pooled detection with the producer's change mask (pH x pW, this frame): a pooled pixel none of whose window pixels the
// producing layer rewrote compares exactly as it did last frame, i.e. not above the threshold.  The 64 pooled pixels of
// word `tile` of row y lie under four words of that mask: false if none of them has a bit set (wave-uniform).
__device__ __forceinline__ bool cb_producer_touched(const unsigned long long* __restrict__ prodMask, int pH, int pW, int y,
                                                    int tile) {
    const int pwpr = (pW + 63) >> 6;
    unsigned long long any = 0ull;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {      // (clamped, not predicated: one round trip for the four)
            const int yy = 2 * y + j, ww = 2 * tile + i;
            const unsigned long long v = prodMask[(long)min(yy, pH - 1) * pwpr + min(ww, pwpr - 1)];
            any |= (yy < pH && ww < pwpr) ? v : 0ull;
        }
    return __builtin_amdgcn_readfirstlane((int)(any != 0ull)) != 0;
}

// The 2x2 max of the pool's input at window corner q by four UNCONDITIONAL loads: px1 / py1 are the offsets of the
// window's second column / row, 0 where the map's edge cuts it off (min(x0 + 1, pW - 1) - x0 and the like) -- such a
// window reads a pixel twice, max(a, a) = a.  A per-lane `if (inside)` around the loads is a branch region of its own for
// every channel, and the compiler then waits for one channel's window before it requests the next.
template <typename T>
__device__ __forceinline__ T cb_pooled_load(const T* q, int px1, int py1) {
    return cb_max(cb_max(q[0], q[px1]), cb_max(q[py1], q[py1 + px1]));
}

// Frame-mask protocol, end of a launch that consumed the frame's mask: ctl = {parity, arrivals} behind the two masks.
// Called by every one of the launch's `groups` workgroups once it has read the parity `par` and its words of the mask;
// the last one to arrive flips the parity and leaves the arrival counter at zero.
__device__ __forceinline__ void cb_flip_parity_last(int* ctl, int par, int groups) {
    __syncthreads();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(ctl + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1) {
        __hip_atomic_store(ctl + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ctl, par ^ 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// x = hi + mid + lo with three bf16 terms (24 significant bits): hi = bf16(x), mid = bf16(x - hi),
// lo = bf16(x - hi - mid); both differences are exact in f32.  Returned as the raw 16-bit patterns.
// (cbs_split3 in cb_split_common.h is NOT a copy: it carries non-finite inputs and truncates near FLT_MAX.)
__device__ __forceinline__ void cb_split3(float x, unsigned& hi, unsigned& mid, unsigned& lo) {
    const __bf16 h = (__bf16)x;
    const float r1 = x - (float)h;
    const __bf16 m = (__bf16)r1;
    const float r2 = r1 - (float)m;
    const __bf16 l = (__bf16)r2;
    hi = __builtin_bit_cast(unsigned short, h);
    mid = __builtin_bit_cast(unsigned short, m);
    lo = __builtin_bit_cast(unsigned short, l);
}

// A kernel whose arguments are a struct of several hundred bytes reads them where it needs them: a handful of
// scalar loads at a time, each group a round trip to the kernel-argument memory (which misses the scalar cache
// the first time a 64-byte line is touched), one after the other along the kernel's critical path.  This touches
// every line of the first BYTES argument bytes in ONE burst at kernel entry, so that all later reads hit.
template <int BYTES>
__device__ __forceinline__ void cb_touch_kernarg() {
    const cb_const_int* ka = (const cb_const_int*)__builtin_amdgcn_kernarg_segment_ptr();
    int acc = 0;
#pragma unroll
    for (int o = 0; o < BYTES; o += 64) acc |= ka[o / 4];
    asm volatile("" ::"s"(acc));
}
