// Change-based max and average pooling for any window, stride, zero padding and ceil_mode on gfx950.
// The reference pools 2x2/stride-2 windows only (cbconv2d_cg_backend.cu:199-240, cb_pool_fg.hip here); contracts of the
// entry points in include/cbinfer_hip.h.  A frame is two launches on the caller's stream:
//   footprint  the output pixels whose window, clipped to the input map, holds a changed input pixel, ORed into a
//              zeroed row-padded bit mask of the OUTPUT map -- from the producer's change LIST (one thread per entry and
//              output row it reaches, at most two 64-bit atomicOr per row) or from its change MASK (one wave per output
//              mask word, one ballot, no atomics);
//   pooling    mask-driven: workgroups of four waves stride over the output mask words, the (set bit, channel) items of
//              a non-empty word spread over the 256 threads (cb_walk_items of cb_maskwalk.h).  The word's owner copies
//              it to the frame's mask copy and zeroes it in the working mask for the next frame.
// No host sync, memset, allocation, data atomics or inline assembly.
#include <math.h>

#include "cb_maskwalk.h"

namespace {

#define CBP2_MAXK 8      // window and stride limit per axis

// first / last output coordinate whose window [o s - p, o s - p + k) holds input coordinate v, clipped to [0, n)
__device__ __forceinline__ void cbp2_reach(int v, int k, int s, int p, int n, int& lo, int& hi) {
    const int t = v + p - k + 1;
    lo = t <= 0 ? 0 : (t + s - 1) / s;
    hi = min((v + p) / s, n - 1);
}

// List form: one thread per (list entry, r-th output row the entry reaches), r < R = ceil(kH / sH).  The columns the
// entry reaches are a run of at most kW <= 8 consecutive bits: at most two words.
__global__ __launch_bounds__(256) void cbp2_footprint_list_kernel(const int32_t* __restrict__ list, int nHost,
                                                                 const int32_t* __restrict__ countDev, int Hi, int Wi,
                                                                 int Ho, int Wo, int wprO, cbPool g, int R,
                                                                 unsigned long long* __restrict__ bits) {
    const int N = countDev ? min(*countDev, nHost) : nHost;
    const long total = (long)N * R;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / R), r = (int)(i - (long)n * R);
        const int pos = list[n];
        if ((unsigned)pos >= (unsigned)(Hi * Wi)) continue;      // (an out-of-map entry is dropped)
        const int y = pos / Wi, x = pos - y * Wi;
        int oyLo, oyHi, oxLo, oxHi;
        cbp2_reach(y, g.kH, g.sH, g.pH, Ho, oyLo, oyHi);
        const int oy = oyLo + r;
        if (oy > oyHi) continue;
        cbp2_reach(x, g.kW, g.sW, g.pW, Wo, oxLo, oxHi);
        if (oxLo > oxHi) continue;                               // (s > k: the pixel lies in a gap between windows)
        const int w0 = oxLo >> 6, w1 = oxHi >> 6;
        const unsigned long long lo = ~0ull << (oxLo & 63), hi = ~0ull >> (63 - (oxHi & 63));
        if (w0 == w1) {
            atomicOr(bits + (long)oy * wprO + w0, lo & hi);
        } else {
            atomicOr(bits + (long)oy * wprO + w0, lo);
            atomicOr(bits + (long)oy * wprO + w1, hi);
        }
    }
}

// Mask form: one wave per output mask word (oy, w).  Lane j owns output column 64 w + j and tests the at most kW input
// bits of its window (at most two input words) in each of the at most kH input rows; one ballot makes the word, which
// only this wave touches.
__global__ __launch_bounds__(256) void cbp2_footprint_mask_kernel(const unsigned long long* __restrict__ inMask, int Hi,
                                                                 int Wi, int wprI, int Ho, int Wo, int wprO, cbPool g,
                                                                 unsigned long long* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const long word = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (word >= (long)Ho * wprO) return;      // uniform over the wave
    const int oy = (int)(word / wprO), w = (int)(word - (long)oy * wprO);
    const int ox = w * 64 + lane;
    bool bit = false;
    if (ox < Wo) {
        const int x0 = ox * g.sW - g.pW, y0 = oy * g.sH - g.pH;
        const int xl = max(x0, 0), xh = min(x0 + g.kW, Wi) - 1;
        const int yl = max(y0, 0), yh = min(y0 + g.kH, Hi) - 1;
        if (xl <= xh) {
            const int w0 = xl >> 6, w1 = xh >> 6;
            const unsigned long long lo = ~0ull << (xl & 63), hi = ~0ull >> (63 - (xh & 63));
            for (int y = yl; y <= yh; ++y) {
                const unsigned long long* row = inMask + (long)y * wprI;
                if (w0 == w1)
                    bit |= (row[w0] & lo & hi) != 0;
                else
                    bit |= ((row[w0] & lo) | (row[w1] & hi)) != 0;
            }
        }
    }
    const unsigned long long m = __ballot(bit);
    if (lane == 0 && m) bits[word] |= m;
}

// Pooling driven by the mask.  OP 0: max, 1: average, divisor counts the padding, 2: average over the in-map pixels.
// The average is summed in f32 in row-major window order and divided once (IEEE division), then rounded to T once.
// The outer loop is this kernel's own, not cb_walk_words: cbinfer_pool_changed copies every word of `bits` to maskCopy AS
// IT IS, row-padding bits a caller set included (they are skipped per item), where the walk cuts the word to the row.
template <typename T, int OP>
__global__ __launch_bounds__(256) void cbp2_pool_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                       unsigned long long* bits, unsigned long long* __restrict__ maskCopy,
                                                       long words, int C, int Hi, int Wi, int Ho, int Wo, int wprO,
                                                       cbPool g) {
    const long HWi = (long)Hi * Wi, HWo = (long)Ho * Wo;
    for (long w = blockIdx.x; w < words; w += gridDim.x) {
        // (uniform over the workgroup: the word is zeroed only behind the barrier below)
        const unsigned long long word = bits[w];
        if (threadIdx.x == 0) maskCopy[w] = word;
        if (word == 0) continue;
        const int oy = (int)(w / wprO), xBase = (int)(w - (long)oy * wprO) * 64;
        const int y0 = oy * g.sH - g.pH;
        const int yl = max(y0, 0), yh = min(y0 + g.kH, Hi);
        cb_walk_items(word, C, [&](int c, int bit) {
            const int ox = xBase + bit;
            if (ox >= Wo) return;      // (a bit of the row padding: never set by the footprint launches)
            const int x0 = ox * g.sW - g.pW;
            const int xl = max(x0, 0), xh = min(x0 + g.kW, Wi);
            const T* src = in + (long)c * HWi;
            T res;
            if (OP == 0) {
                // torch's max rule (max_pool2d: a later value wins only if greater; a NaN wins always)
                float v = -INFINITY;
                for (int y = yl; y < yh; ++y)
                    for (int x = xl; x < xh; ++x) {
                        const float t = cb_load_f32(src + (long)y * Wi + x);
                        if (t > v || t != t) v = t;
                    }
                res = (T)v;      // (exact: v is one of the inputs, or -inf for an empty window)
            } else {
                float sum = 0.f;
                for (int y = yl; y < yh; ++y)
                    for (int x = xl; x < xh; ++x) sum += cb_load_f32(src + (long)y * Wi + x);
                const int div = OP == 1 ? (min(y0 + g.kH, Hi + g.pH) - y0) * (min(x0 + g.kW, Wi + g.pW) - x0)
                                        : (yh - yl) * (xh - xl);
                res = (T)__fdiv_rn(sum, (float)div);
            }
            out[(long)c * HWo + (long)oy * Wo + ox] = res;
        });
        __syncthreads();      // every wave has read the word
        if (threadIdx.x == 0) bits[w] = 0;
    }
}

int cbp2_axis_out(int n, int k, int s, int p, int ceilMode) {
    const int num = n + 2 * p - k;
    if (num < 0) return 0;
    int o = (ceilMode ? (num + s - 1) / s : num / s) + 1;
    if (ceilMode && (o - 1) * s >= n + p) --o;
    return o;
}

template <typename T>
void cbp2_launch_pool(const void* input, void* output, uint64_t* bits, uint64_t* maskCopy, long words, int C, int Hi,
                      int Wi, int Ho, int Wo, const cbPool& g, hipStream_t s) {
    const dim3 grid(cb_walk_grid(words)), block(256);
    const int wprO = (Wo + 63) / 64;
#define CBP2_GO(OP)                                                                                                   \
    hipLaunchKernelGGL((cbp2_pool_kernel<T, OP>), grid, block, 0, s, (const T*)input, (T*)output,                    \
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, C, Hi, Wi, Ho, Wo, wprO, g)
    if (g.op == CB_POOL_MAX)
        CBP2_GO(0);
    else if (g.op == CB_POOL_AVG_PAD)
        CBP2_GO(1);
    else
        CBP2_GO(2);
#undef CBP2_GO
}

}  // namespace

int cbinfer_pool_supported(const cbPool* pool) {
    if (!pool) return 0;
    const cbPool& g = *pool;
    return g.kH >= 1 && g.kW >= 1 && g.kH <= CBP2_MAXK && g.kW <= CBP2_MAXK && g.sH >= 1 && g.sW >= 1 &&
           g.sH <= CBP2_MAXK && g.sW <= CBP2_MAXK && g.pH >= 0 && g.pW >= 0 && 2 * g.pH <= g.kH && 2 * g.pW <= g.kW &&
           (g.ceilMode == 0 || g.ceilMode == 1) && g.op >= CB_POOL_MAX && g.op <= CB_POOL_AVG_NOPAD;
}

int cbinfer_pool_out_size(int Hi, int Wi, const cbPool* pool, int* Ho, int* Wo) {
    CB_REQUIRE(pool && Ho && Wo && Hi > 0 && Wi > 0);
    if (!cbinfer_pool_supported(pool)) return CB_ERR_UNSUPPORTED;
    const int ho = cbp2_axis_out(Hi, pool->kH, pool->sH, pool->pH, pool->ceilMode);
    const int wo = cbp2_axis_out(Wi, pool->kW, pool->sW, pool->pW, pool->ceilMode);
    CB_REQUIRE(ho > 0 && wo > 0);      // (a map smaller than the window: refused)
    *Ho = ho, *Wo = wo;
    return CB_OK;
}

int cbinfer_pool_footprint(const int32_t* changeIndexes, int capN, const int32_t* countDev, const uint64_t* inputMask,
                           int Hi, int Wi, const cbPool* pool, uint64_t* bits, cbStream_t stream) {
    CB_REQUIRE(bits && (changeIndexes != nullptr) != (inputMask != nullptr) && capN >= 0);
    CB_REQUIRE(!inputMask || !countDev);
    int Ho, Wo;
    const int st = cbinfer_pool_out_size(Hi, Wi, pool, &Ho, &Wo);
    if (st != CB_OK) return st;
    CB_REQUIRE((long)Hi * Wi < (1l << 31));
    const int wprO = (Wo + 63) / 64;
    if (inputMask) {
        const long words = (long)Ho * wprO;
        hipLaunchKernelGGL(cbp2_footprint_mask_kernel, dim3((unsigned)((words + 3) / 4)), dim3(256), 0,
                           (hipStream_t)stream, (const unsigned long long*)inputMask, Hi, Wi, (Wi + 63) / 64, Ho, Wo,
                           wprO, *pool, (unsigned long long*)bits);
        return cb_launch_status();
    }
    if (capN == 0) return CB_OK;
    const int R = (pool->kH + pool->sH - 1) / pool->sH;
    long blocks = ((long)capN * R + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(cbp2_footprint_list_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       changeIndexes, capN, countDev, Hi, Wi, Ho, Wo, wprO, *pool, R, (unsigned long long*)bits);
    return cb_launch_status();
}

int cbinfer_pool_changed(const void* input, void* output, uint64_t* bits, uint64_t* maskCopy, int C, int Hi, int Wi,
                         const cbPool* pool, int dtype, cbStream_t stream) {
    CB_REQUIRE(input && output && bits && maskCopy && bits != maskCopy && C > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    int Ho, Wo;
    const int st = cbinfer_pool_out_size(Hi, Wi, pool, &Ho, &Wo);
    if (st != CB_OK) return st;
    // (the kernel numbers a word's items with an int)
    CB_REQUIRE((long)C * 64 < (1l << 31));
    const long words = (long)Ho * ((Wo + 63) / 64);
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbp2_launch_pool<decltype(t)>(input, output, bits, maskCopy, words, C, Hi, Wi, Ho, Wo, *pool, (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbpool2d_forward(const void* input, void* outputState, const int32_t* changeIndexes, int capN,
                             const int32_t* countDev, const uint64_t* inputMask, uint64_t* bits, uint64_t* maskCopy,
                             int C, int Hi, int Wi, const cbPool* pool, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && outputState && bits && maskCopy && bits != maskCopy && C > 0 && capN >= 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE((changeIndexes != nullptr) != (inputMask != nullptr) && (!inputMask || !countDev));
    CB_REQUIRE((long)C * 64 < (1l << 31));
    int st = cbinfer_pool_footprint(changeIndexes, capN, countDev, inputMask, Hi, Wi, pool, bits, stream);
    if (st != CB_OK) return st;
    return cbinfer_pool_changed(input, outputState, bits, maskCopy, C, Hi, Wi, pool, dtype, stream);
}
