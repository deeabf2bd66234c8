// Change-based adaptive and global pooling, max and average, on gfx950: torch's nn.AdaptiveMaxPool2d /
// nn.AdaptiveAvgPool2d behind a producer.  Specification and contracts of the entry points in include/cbinfer_hip.h.
// A window of a global pool is the whole map, so recomputing a listed output pixel from its window (cb_pool2d.hip) would
// cost the dense operator for one changed pixel.  Here a second level of state stands between input and output: the
// row-segment partials P[C][ow][H] (f32).  A frame is two launches on the caller's stream (three for a list):
//   partials  unit = (input row, block of 32 channels) on a persistent grid.  A unit forms the dirty column windows of
//             its row from the row's mask words -- one ballot per 64 windows --, recomputes the partials of those windows
//             with L lanes along x per segment (fixed lane tree), and its first channel block ORs the dirty windows into
//             the one or two output rows that hold the input row: one 64-bit atomicOr per dirty (row, output word).
//   changed   one workgroup per word of the output mask: an item (c, i, j) reduces the rows of its window -- consecutive
//             floats of P -- on L2 lanes in the same fixed order and writes the output; the word's owner stores the
//             mask copy and zeroes the working word.
// Both levels run cbap_reduce, several items side by side on a group of lanes, so that their loads overlap.
// A partial has ONE writer: the owner of (row, channel block) -- a column window may span mask words (W = 70, ow = 1).
// No host sync, allocation, inter-workgroup waiting, data atomics or inline assembly.
#include <limits.h>
#include <math.h>

#include "cb_maskwalk.h"

namespace {

#define CBAP_MAXWORDS 64      // words of one row of the output mask a workgroup keeps: ow <= 4096
#define CBAP_CHUNK 32         // channels per unit of the partials launch
// items a group of lanes reduces side by side, and steps of the lane sum whose loads are issued together: the partials
// launch has many workgroups, the second launch one per mask word
#define CBAP_UA 4
#define CBAP_KA 4
#define CBAP_UB 8
#define CBAP_KB 2

// torch's adaptive window of output coordinate i on an N-long axis pooled to o: [lo, hi).  In 32 bits: the entry points
// refuse an axis with (N + 1) o beyond an int32.
__host__ __device__ __forceinline__ int cbap_lo(int i, int N, int o) {
    return (int)((unsigned)i * (unsigned)N / (unsigned)o);
}
__host__ __device__ __forceinline__ int cbap_hi(int i, int N, int o) {
    return (int)((((unsigned)i + 1u) * (unsigned)N + (unsigned)o - 1u) / (unsigned)o);
}

// lanes of a reduction along an axis: the smallest power of two >= the longest window the axis can have, at most 64
int cbap_lanes(int N, int o) {
    if (N < 1 || o < 1 || o > N) return 1;
    const int nmax = N % o == 0 ? N / o : N / o + 2;
    int L = 1;
    while (L < nmax && L < 64) L *= 2;
    return L;
}

// One level of the header's order for U items at once on the L lanes of a group (lane l of it): item u's values are
// load(u, 0) ... load(u, len[u] - 1), first to last, len[u] >= 1.  Returns item u's result in res[u] on lane 0 of the
// group.  The items' loads are independent and issued KU steps of the lane sum ahead, so that they overlap: a step is
// a round trip to memory, and a workgroup has few of them to hide it behind.
//   sum      s_l = +0, s_l += x_k for k = l, l + L, ... < len ascending; then s_l += s_(l + off) for off = L / 2 ... 1
//            (a value behind the item's end is read again from its last element and counts as +0, which changes nothing:
//            a lane sum that began at +0 is never -0)
//   maximum  (value, position): a later value of the lane wins only if greater (a NaN always); in the tree, of two equal
//            values the one that comes first
template <int OP, int U, int KU, typename Load>
__device__ __forceinline__ void cbap_reduce(Load load, const int (&len)[U], int l, int L, float (&res)[U]) {
    int at[U], n = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) res[u] = OP == CB_ADAPT_AVG ? 0.f : -INFINITY, at[u] = INT_MAX, n = max(n, len[u]);
    for (int k0 = l; k0 < n; k0 += L * KU) {
        float t[KU][U];
#pragma unroll
        for (int q = 0; q < KU; ++q)
#pragma unroll
            for (int u = 0; u < U; ++u) t[q][u] = load(u, min(k0 + q * L, len[u] - 1));
#pragma unroll
        for (int q = 0; q < KU; ++q)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + q * L;
                const bool ok = k < len[u];
                if (OP == CB_ADAPT_AVG)
                    res[u] += ok ? t[q][u] : 0.f;
                else if (ok && (at[u] == INT_MAX || t[q][u] > res[u] || t[q][u] != t[q][u]))
                    res[u] = t[q][u], at[u] = k;
            }
    }
    for (int off = L >> 1; off >= 1; off >>= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float t = __shfl_down(res[u], off, L);
            if (OP == CB_ADAPT_AVG) {
                res[u] += t;
            } else {
                const int tat = __shfl_down(at[u], off, L);
                if (res[u] == res[u] && (t != t || t > res[u] || (t == res[u] && tat < at[u]))) res[u] = t, at[u] = tat;
            }
        }
    }
}

// the r-th set bit of the `words` words at `bits` (r < their popcount), as a bit position over all of them
__device__ __forceinline__ int cbap_select(const unsigned long long* bits, int words, int r) {
    for (int t = 0; t < words; ++t) {
        const int n = __popcll(bits[t]);
        if (r < n) return t * 64 + (n == 64 ? r : cb_select_bit(bits[t], r));
        r -= n;
    }
    return 0;
}

template <typename T, int OP>
__global__ __launch_bounds__(256) void cbap_partials_kernel(const T* __restrict__ in, float* __restrict__ P,
                                                           const unsigned long long* __restrict__ inMask,
                                                           const unsigned long long* __restrict__ inBits, int all,
                                                           unsigned long long* outBits, int C, int H, int W, int oh, int ow,
                                                           int L, int chunks) {
    __shared__ unsigned long long dirty[CBAP_MAXWORDS];
    __shared__ unsigned short wj[CBAP_MAXWORDS * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wprI = (W + 63) >> 6, wprO = (ow + 63) >> 6;
    const int groups = 256 / L, g = threadIdx.x / L, l = threadIdx.x & (L - 1);
    const long units = (long)H * chunks;
    for (long u = blockIdx.x; u < units; u += gridDim.x) {      // (uniform over the workgroup)
        const int y = (int)(u / chunks), chunk = (int)(u - (long)y * chunks);
        // the dirty column windows of row y: lane = window, one ballot per 64 of them
        for (int jb = wave * 64; jb < wprO * 64; jb += 256) {
            const int j = jb + lane;
            bool d = false;
            if (j < ow) {
                if (all) {
                    d = true;
                } else {
                    const int x0 = cbap_lo(j, W, ow), xl = cbap_hi(j, W, ow) - 1;      // first and last column
                    const int w0 = x0 >> 6, w1 = xl >> 6;
                    for (int t = w0; t <= w1; ++t) {
                        unsigned long long word = inMask ? inMask[(long)y * wprI + t] : 0ull;
                        if (inBits) word |= inBits[(long)y * wprI + t];
                        if (t == w0) word &= ~0ull << (x0 & 63);
                        if (t == w1) word &= ~0ull >> (63 - (xl & 63));
                        d |= word != 0ull;
                    }
                }
            }
            const unsigned long long m = __ballot(d);
            if (lane == 0) dirty[jb >> 6] = m;
        }
        __syncthreads();
        int nd = 0;
        for (int t = 0; t < wprO; ++t) nd += __popcll(dirty[t]);
        if (nd != 0) {
            if (chunk == 0) {
                // footprint: the windows' bits in the one or two output rows whose window holds y
                const int iLo = cbap_lo(y, oh, H), iHi = cbap_hi(y, oh, H) - 1;
                for (int q = threadIdx.x; q < wprO * (iHi - iLo + 1); q += 256) {
                    const int t = q % wprO, i = iLo + q / wprO;
                    if (dirty[t] != 0ull) atomicOr(outBits + (long)i * wprO + t, dirty[t]);
                }
            }
            // the dirty windows once, in LDS; an item is (channel, dirty window), window fastest, and a group steps
            // through them `groups` at a time without a division per item
            for (int r = threadIdx.x; r < nd; r += 256) wj[r] = (unsigned short)cbap_select(dirty, wprO, r);
            __syncthreads();
            const int c0 = chunk * CBAP_CHUNK, cn = min(C - c0, CBAP_CHUNK);
            const int qd = groups / nd, rd = groups - qd * nd;
            int c = g / nd, r = g - c * nd;
            while (c < cn) {      // (uniform over the lanes of a group)
                const T* src[CBAP_UA];
                int dst[CBAP_UA], len[CBAP_UA];      // (the windows of the items may differ in length)
#pragma unroll
                for (int k = 0; k < CBAP_UA; ++k) {
                    const int cc = c0 + min(c, cn - 1), j = wj[r];      // (behind the last item: a channel of the last one)
                    const int x0 = cbap_lo(j, W, ow);
                    src[k] = in + ((long)cc * H + y) * W + x0;
                    dst[k] = c < cn ? (cc * ow + j) * H + y : -1;
                    len[k] = cbap_hi(j, W, ow) - x0;
                    c += qd, r += rd;
                    if (r >= nd) r -= nd, ++c;
                }
                float res[CBAP_UA];
                cbap_reduce<OP, CBAP_UA, CBAP_KA>([&](int k, int x) { return cb_load_f32(src[k] + x); }, len, l, L, res);
#pragma unroll
                for (int k = 0; k < CBAP_UA; ++k)
                    if (l == 0 && dst[k] >= 0) P[dst[k]] = res[k];
            }
        }
        __syncthreads();      // every thread has read `dirty` before the next unit writes it
    }
}

// Launch 2: one workgroup of 1024 threads per non-empty word of the output mask; the items (channel, set bit), bit
// fastest, go to groups of L2 lanes, which reduce the rows of the window -- consecutive floats of P[C][ow][H].
template <typename T, int OP>
__global__ __launch_bounds__(1024) void cbap_changed_kernel(const float* __restrict__ P, T* __restrict__ out,
                                                           unsigned long long* __restrict__ inBits, long wordsI,
                                                           unsigned long long* outBits,
                                                           unsigned long long* __restrict__ maskCopy, long words, int C,
                                                           int H, int W, int oh, int ow, int wprO, int L2) {
    // (list form: the working mask of the input map, which the partials launch only read)
    if (inBits)
        for (long w = (long)blockIdx.x * 1024 + threadIdx.x; w < wordsI; w += (long)gridDim.x * 1024) inBits[w] = 0ull;
    __shared__ int pos[64];
    const int groups = 1024 / L2, g = threadIdx.x / L2, l = threadIdx.x & (L2 - 1);
    for (long w = blockIdx.x; w < words; w += gridDim.x) {
        // (uniform over the workgroup: the word is zeroed only behind the barrier below)
        const unsigned long long own = outBits[w];
        const int i = (int)(w / wprO), tile = (int)(w - (long)i * wprO);
        const unsigned long long word = own & cb_valid_mask(ow, tile);      // (the bits of the row padding are never set)
        if (threadIdx.x == 0) maskCopy[w] = word;
        if (word != 0ull) {
            // the word's columns once, in LDS; an item is (channel, set bit), bit fastest, and a group steps through them
            // `groups` at a time without a division per item
            const int nb = __popcll(word);
            if ((int)threadIdx.x < nb) pos[threadIdx.x] = tile * 64 + (nb == 64 ? (int)threadIdx.x : cb_select_bit(word, threadIdx.x));
            __syncthreads();
            const int r0 = cbap_lo(i, H, oh), rows = cbap_hi(i, H, oh) - r0;
            const int qd = groups / nb, rd = groups - qd * nb;
            int c = g / nb, b = g - c * nb;
            while (c < C) {      // (uniform over the lanes of a group)
                int src[CBAP_UB], dst[CBAP_UB], cols[CBAP_UB], len[CBAP_UB];
#pragma unroll
                for (int k = 0; k < CBAP_UB; ++k) {
                    const int cc = min(c, C - 1), j = pos[b];      // (behind the last item: a channel of the last one again)
                    src[k] = (cc * ow + j) * H + r0;
                    dst[k] = c < C ? (cc * oh + i) * ow + j : -1;
                    cols[k] = cbap_hi(j, W, ow) - cbap_lo(j, W, ow);
                    len[k] = rows;
                    c += qd, b += rd;
                    if (b >= nb) b -= nb, ++c;
                }
                float res[CBAP_UB];
                cbap_reduce<OP, CBAP_UB, CBAP_KB>([&](int k, int r) { return P[src[k] + r]; }, len, l, L2, res);
#pragma unroll
                for (int k = 0; k < CBAP_UB; ++k)
                    if (l == 0 && dst[k] >= 0)
                        out[dst[k]] = (T)(OP == CB_ADAPT_AVG ? __fdiv_rn(res[k], (float)(rows * cols[k])) : res[k]);
            }
        }
        if (own != 0ull) {
            __syncthreads();      // every wave has read the word
            if (threadIdx.x == 0) outBits[w] = 0ull;
        }
    }
}

int cbap_shape_status(int C, int H, int W, int oh, int ow) {
    CB_REQUIRE(C >= 1 && H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && oh <= H && ow <= W);
    // (a list addresses a pixel with an int32; the walk numbers a word's items with an int)
    if (ow > CBAP_MAXWORDS * 64 || (long)H * W >= (1l << 31) || (long)C * 64 >= (1l << 31) ||
        (long)C * H * ow >= (1l << 31) || ((long)H + 1) * oh >= (1l << 31) || ((long)W + 1) * ow >= (1l << 31))
        return CB_ERR_UNSUPPORTED;
    return CB_OK;
}

bool cbap_kind_ok(int op, int dtype) {
    return (op == CB_ADAPT_MAX || op == CB_ADAPT_AVG) && (dtype == CB_F32 || dtype == CB_F16);
}

}  // namespace

int cbinfer_adaptive_pool_supported(int H, int W, int oh, int ow) { return cbap_shape_status(1, H, W, oh, ow) == CB_OK; }

int cbinfer_adaptive_pool_lanes(int N, int o) { return cbap_lanes(N, o); }

long cbinfer_adaptive_pool_partial_elems(int C, int H, int W, int oh, int ow) {
    return cbap_shape_status(C, H, W, oh, ow) == CB_OK ? (long)C * H * ow : 0;
}

int cbinfer_adaptive_pool_partials(const void* input, float* partials, const uint64_t* inputMask, const uint64_t* inBits,
                                   int all, uint64_t* outBits, int C, int H, int W, int oh, int ow, int op, int dtype,
                                   cbStream_t stream) {
    CB_REQUIRE(input && partials && outBits && (inputMask || inBits || all) && cbap_kind_ok(op, dtype));
    CB_REQUIRE(input != (const void*)partials && inputMask != outBits && inBits != outBits);
    const int st = cbap_shape_status(C, H, W, oh, ow);
    if (st != CB_OK) return st;
    const int chunks = (C + CBAP_CHUNK - 1) / CBAP_CHUNK, L = cbap_lanes(W, ow);
    const dim3 grid(cb_walk_grid((long)H * chunks)), block(256);
    cb_dispatch_dtype(dtype, [&](auto t) {
        typedef decltype(t) T;
#define CBAP_GO(OP)                                                                                                   \
    hipLaunchKernelGGL((cbap_partials_kernel<T, OP>), grid, block, 0, (hipStream_t)stream, (const T*)input, partials, \
                       (const unsigned long long*)inputMask, (const unsigned long long*)inBits, all,                  \
                       (unsigned long long*)outBits, C, H, W, oh, ow, L, chunks)
        if (op == CB_ADAPT_MAX)
            CBAP_GO(CB_ADAPT_MAX);
        else
            CBAP_GO(CB_ADAPT_AVG);
#undef CBAP_GO
    });
    return cb_launch_status();
}

int cbinfer_adaptive_pool_changed(const float* partials, void* output, uint64_t* inBits, uint64_t* outBits,
                                  uint64_t* maskCopy, int C, int H, int W, int oh, int ow, int op, int dtype,
                                  cbStream_t stream) {
    CB_REQUIRE(partials && output && outBits && maskCopy && cbap_kind_ok(op, dtype));
    CB_REQUIRE((const void*)partials != output && outBits != maskCopy && inBits != outBits && inBits != maskCopy);
    const int st = cbap_shape_status(C, H, W, oh, ow);
    if (st != CB_OK) return st;
    const int wprO = (ow + 63) / 64;
    const long words = (long)oh * wprO, wordsI = (long)H * ((W + 63) / 64);
    const int L2 = cbap_lanes(H, oh);
    const dim3 grid(cb_walk_grid(words)), block(1024);
    cb_dispatch_dtype(dtype, [&](auto t) {
        typedef decltype(t) T;
#define CBAP_GO(OP)                                                                                                  \
    hipLaunchKernelGGL((cbap_changed_kernel<T, OP>), grid, block, 0, (hipStream_t)stream, partials, (T*)output,      \
                       (unsigned long long*)inBits, wordsI, (unsigned long long*)outBits,                            \
                       (unsigned long long*)maskCopy, words, C, H, W, oh, ow, wprO, L2)
        if (op == CB_ADAPT_MAX)
            CBAP_GO(CB_ADAPT_MAX);
        else
            CBAP_GO(CB_ADAPT_AVG);
#undef CBAP_GO
    });
    return cb_launch_status();
}

int cbinfer_cbadaptivepool2d_forward(const void* input, float* partials, void* outputState, const uint64_t* inputMask,
                                     const int32_t* changeIndexes, int capN, const int32_t* countDev, uint64_t* inBits,
                                     uint64_t* outBits, uint64_t* maskCopy, int C, int H, int W, int oh, int ow, int op,
                                     int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && partials && outputState && outBits && maskCopy && cbap_kind_ok(op, dtype));
    CB_REQUIRE(capN >= 0 && !(inputMask && changeIndexes) && (changeIndexes || !countDev) && (!changeIndexes || inBits));
    CB_REQUIRE(input != outputState && input != (const void*)partials && (const void*)partials != outputState);
    CB_REQUIRE(outBits != maskCopy && inBits != outBits && inBits != maskCopy && inputMask != outBits &&
               inputMask != maskCopy && (!inputMask || inputMask != inBits));
    int st = cbap_shape_status(C, H, W, oh, ow);
    if (st != CB_OK) return st;
    uint64_t* listBits = changeIndexes ? inBits : nullptr;
    if (changeIndexes) {
        st = cb_list_to_bits(changeIndexes, capN, countDev, H, W, listBits, stream);
        if (st != CB_OK) return st;
    }
    st = cbinfer_adaptive_pool_partials(input, partials, inputMask, listBits, !inputMask && !changeIndexes, outBits, C, H,
                                        W, oh, ow, op, dtype, stream);
    if (st != CB_OK) return st;
    return cbinfer_adaptive_pool_changed(partials, outputState, listBits, outBits, maskCopy, C, H, W, oh, ow, op, dtype,
                                         stream);
}
