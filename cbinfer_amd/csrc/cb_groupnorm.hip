// Change-based group norm and instance norm on gfx950: nn.GroupNorm, nn.InstanceNorm2d without running
// statistics (G == C) and GroupNorm(1, C) as a link of the change-based chain.  The reference has no such operator;
// contracts of the entry points and the arithmetic in include/cbinfer_hip.h.  Two halves this library already has are
// combined: a second level of state (5.26) -- f64 partial sums over the segments of a row, one segment per word of the
// change mask, so that a changed pixel costs its segment and not the map -- and the threshold rule on a small per-frame
// vector (5.28): a group whose (mean, rstd) moved by no more than `threshold` keeps the pair it last used (`held`); one
// that moved by more TRIPPED, takes the new pair and has its planes recomputed completely.  A frame is
//   for an operand in LIST form, one launch in front: the list's bits ORed into the zeroed working mask
//              (cb_list_to_bits of cb_maskwalk.h);
//   launch 1   cbgn_partials_kernel, a persistent grid over (mask word, block of 16 channels): the partials of the dirty
//              segments, the f64 butterfly over the 64 lanes;
//   launch 2   cbgn_stats_kernel, ONE workgroup of 1024 threads per group: the sums of the group's partials in the
//              written order, mean and rstd in f64, the trip decision, `held` and tripped[g];
//   launch 3   cbgn_apply_kernel, the word walk of cb_maskwalk.h (cb_walk_word_units): every channel at a listed pixel,
//              the channels of the tripped groups at every other pixel.
// Three launches: the readers of the partials and of `held` must not share a launch with their writers.  No atomics,
// host sync, memset, allocation or inline assembly; all stores are plain vector stores.
#include <math.h>

#include "cb_maskwalk.h"

// every product and sum below is rounded on its own, in the order written (as cb_pointwise.hip)
#pragma clang fp contract(off)

namespace {

constexpr int CBGN_MAX_C = 4096;
constexpr int CBGN_BLOCK = 16;      // channels per unit of launch 1: four per wave, their loads in flight together
constexpr int CBGN_STAT_THREADS = 1024;

// p_l + p_(l xor m), m = 1 ... 32: the fixed butterfly of the specification (an IEEE sum does not depend on the order
// of its two operands, so every lane ends with the same value)
__device__ __forceinline__ double cbgn_butterfly(double p) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) p = p + __shfl_xor(p, m, 64);
    return p;
}

// a [C, H, W]; partials [2][C][H][wpr] f64.  Unit u = (word w, channel block): w = u / nblk.  The listed word is only
// read here; launch 3 zeroes the working mask.
template <typename T>
__global__ __launch_bounds__(256) void cbgn_partials_kernel(const T* __restrict__ a, double* __restrict__ partials,
                                                           const unsigned long long* __restrict__ maskA,
                                                           const unsigned long long* __restrict__ bits, int all,
                                                           long words, int nblk, int C, int H, int W, int wpr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long HW = (long)H * W, units = words * nblk;
    for (long u = blockIdx.x; u < units; u += gridDim.x) {
        const long w = u / nblk;
        const int blk = (int)(u - w * nblk);
        const int y = (int)(w / wpr), tile = (int)(w - (long)y * wpr);
        const unsigned long long valid = cb_valid_mask(W, tile);
        const unsigned long long listed =
            all ? valid : (((bits ? bits[w] : 0ull) | (maskA ? maskA[w] : 0ull)) & valid);
        if (listed == 0) continue;      // (uniform over the workgroup: a clean segment is never read)
        const int x = tile * 64 + lane;
        const bool inside = x < W;
        const int c0 = blk * CBGN_BLOCK + wave * (CBGN_BLOCK / 4);
        double v[CBGN_BLOCK / 4];
#pragma unroll
        for (int i = 0; i < CBGN_BLOCK / 4; ++i) {      // (one coalesced 64-lane load per channel, all in flight)
            const int c = c0 + i;
            v[i] = (inside && c < C) ? (double)cb_load_f32(a + (long)c * HW + (long)y * W + x) : 0.0;
        }
#pragma unroll
        for (int i = 0; i < CBGN_BLOCK / 4; ++i) {
            const int c = c0 + i;      // (uniform over the wave: every lane takes part in every butterfly)
            if (c >= C) break;
            const double s1 = cbgn_butterfly(v[i]);
            const double s2 = cbgn_butterfly(v[i] * v[i]);      // (exact in f64)
            if (lane == 0) {
                partials[(long)c * words + w] = s1;
                partials[((long)C + c) * words + w] = s2;
            }
        }
    }
}

// One workgroup of 1024 threads per group g.  stats, held [2][G] f32; tripped [G] int32, every entry written.
__global__ __launch_bounds__(CBGN_STAT_THREADS) void cbgn_stats_kernel(const double* __restrict__ partials,
                                                                      float* __restrict__ stats,
                                                                      float* __restrict__ held,
                                                                      int* __restrict__ tripped, long words, int C, int G,
                                                                      double n, double eps, float threshold, int all) {
    __shared__ double s[2][CBGN_STAT_THREADS];
    const int g = blockIdx.x, tid = threadIdx.x, Cg = C / G;
    const long N = (long)Cg * words;
    const double* p1 = partials + (long)g * Cg * words;
    const double* p2 = partials + ((long)C + (long)g * Cg) * words;
    double s1 = 0.0, s2 = 0.0;
    for (long i = tid; i < N; i += CBGN_STAT_THREADS) {
        s1 = s1 + p1[i];
        s2 = s2 + p2[i];
    }
    s[0][tid] = s1;
    s[1][tid] = s2;
    __syncthreads();
    for (int off = CBGN_STAT_THREADS / 2; off >= 1; off >>= 1) {
        if (tid < off) {
            s[0][tid] = s[0][tid] + s[0][tid + off];
            s[1][tid] = s[1][tid] + s[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double mean64 = s[0][0] / n;
        const double sq = mean64 * mean64;
        double var = s[1][0] / n - sq;
        var = var < 0.0 ? 0.0 : var;      // (a NaN stays)
        const double rstd64 = 1.0 / sqrt(var + eps);
        const float mean = (float)mean64, rstd = (float)rstd64;
        stats[g] = mean;
        stats[G + g] = rstd;
        const float hm = held[g], hr = held[G + g];
        // strictly more than the threshold; a NaN trips
        const bool trip = all || !(fabsf(mean - hm) * hr <= threshold) || !(fabsf(rstd - hr) <= threshold * hr);
        if (trip) {
            held[g] = mean;
            held[G + g] = rstd;
        }
        tripped[g] = trip ? 1 : 0;
    }
}

// (T)v with v = ((x - mean) rstd) gamma + beta, the ReLU: every operation an instruction of its own.  Written plainly,
// hipcc folds the last product or sum and the f16 conversion into ONE v_fma_mix*: one rounding instead of the
// specification's two (cbcs_scaled of cb_chanscale.hip).  Under strict exception semantics they stay apart.
// (The comparison of the ReLU stands outside the strict parts: a comparison under strict exception semantics does not
// get through this compiler's instruction selection.)
__device__ __forceinline__ float cbgn_affine(float x, float mean, float rstd, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, int c) {
#pragma clang fp exceptions(strict)
    const float d = x - mean;
    float v = d * rstd;
    if (gamma) v = v * gamma[c];
    if (beta) v = v + beta[c];
    return v;
}
template <typename T>
__device__ __forceinline__ T cbgn_rounded(float v) {
#pragma clang fp exceptions(strict)
    return (T)v;
}
template <typename T>
__device__ __forceinline__ T cbgn_value(float x, float mean, float rstd, const float* __restrict__ gamma,
                                        const float* __restrict__ beta, int c, int relu) {
    float v = cbgn_affine(x, mean, rstd, gamma, beta, c);
    if (relu) v = v < 0.f ? 0.f : v;      // (-0 and a NaN stay)
    return cbgn_rounded<T>(v);
}

// a, out [C, H, W]; held [2][G] f32 and tripped [G] as launch 2 left them.  maskA: the operand's change mask of this
// frame, or NULL; all: every pixel is listed with every channel.  An operand without a mask has its bits in `bits`
// already (list form) -- or did not change.  In a frame with a tripped group the frame's mask is the full row word; a
// pixel that is not listed is written in the channels of the tripped groups only.
template <typename T>
__global__ __launch_bounds__(256) void cbgn_apply_kernel(const T* __restrict__ a, T* __restrict__ out,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ held,
                                                        const int* __restrict__ tripped,
                                                        const unsigned long long* __restrict__ maskA, int all,
                                                        unsigned long long* bits,
                                                        unsigned long long* __restrict__ maskCopy, long words, int C,
                                                        int G, int H, int W, int wpr, int relu) {
    __shared__ unsigned short groups[CBGN_MAX_C];      // the tripped groups, ascending
    __shared__ unsigned short chans[CBGN_MAX_C];       // their channels, ascending
    __shared__ int counts[256];
    const long HW = (long)H * W;
    const int Cg = C / G, tid = threadIdx.x;
    // The G flags are read once; the lists are made from them alone, cut to the C channels, and n counted from them:
    // whatever the buffer holds, every entry is a channel of the map and the list has n of them.
    const int per = (G + 255) / 256, g0 = tid * per;
    int mine = 0;
    for (int g = g0; g < g0 + per && g < G; ++g) mine += tripped[g] != 0;
    counts[tid] = mine;
    __syncthreads();
    int before = 0, total = 0;
    for (int t = 0; t < 256; ++t) {
        before += t < tid ? counts[t] : 0;
        total += counts[t];
    }
    for (int g = g0; g < g0 + per && g < G; ++g)
        if (tripped[g] != 0) groups[before++] = (unsigned short)g;
    __syncthreads();
    const long nl = (long)total * Cg;
    const int n = (int)(nl < C ? nl : C);
    for (int i = tid; i < n; i += 256) {
        const int k = i / Cg;
        chans[i] = (unsigned short)(groups[k] * Cg + (i - k * Cg));
    }
    __syncthreads();
    const int full = all || total > 0;      // (uniform over the launch: the frame's mask is the full row word)
    unsigned long long listed = 0;
    cb_walk_word_units(
        bits, maskCopy, words, W, wpr, full,
        // (the working word is zeroed only behind the barrier that follows the unit)
        [&](long w, int, int) { return listed = bits[w] | (maskA ? maskA[w] : 0ull); },
        [&](unsigned long long word, int y, int tile) {
            const long first = (long)y * W + tile * 64;      // (H W fits an int: cbgn_shape_ok)
            const unsigned long long every = all ? word : (listed & word);
            cb_walk_items(every, C, [&](int c, int bit) {
                const long o = (long)c * HW + first + bit;
                const int g = c / Cg;
                out[o] = cbgn_value<T>(cb_load_f32(a + o), held[g], held[G + g], gamma, beta, c, relu);
            });
            cb_walk_items(word & ~every, n, [&](int i, int bit) {
                const int c = chans[i];
                const long o = (long)c * HW + first + bit;
                const int g = c / Cg;
                out[o] = cbgn_value<T>(cb_load_f32(a + o), held[g], held[G + g], gamma, beta, c, relu);
            });
        });
}

bool cbgn_shape_ok(int C, int G, int H, int W) {
    // (a list addresses a pixel with an int32)
    return cbinfer_groupnorm_supported(C, G) && H >= 1 && W >= 1 && (long)H * W < (1l << 31);
}

bool cbgn_partials_ok(const void* a, const double* partials, const uint64_t* maskA, const uint64_t* bits, int C, int H,
                      int W, int dtype) {
    return a && partials && (const void*)partials != a && cbgn_shape_ok(C, 1, H, W) &&
           (dtype == CB_F32 || dtype == CB_F16) && (!maskA || maskA != bits) && (const void*)maskA != partials &&
           (const void*)bits != partials;
}

bool cbgn_stats_ok(const double* partials, const float* stats, const float* held, const int32_t* tripped, int C, int G,
                   int H, int W, const double* eps, float threshold) {
    return partials && stats && held && tripped && stats != held && (const void*)stats != partials &&
           (const void*)held != partials && (const void*)tripped != partials && (const void*)tripped != stats &&
           (const void*)tripped != held && cbgn_shape_ok(C, G, H, W) && eps && *eps >= 0.0 && isfinite(*eps) &&
           threshold >= 0.f;      // (a NaN threshold or eps is not >= 0)
}

bool cbgn_apply_ok(const void* a, const void* out, const float* held, const int32_t* tripped, const uint64_t* maskA,
                   const uint64_t* bits, const uint64_t* maskCopy, int C, int G, int H, int W, int relu, int dtype) {
    return a && out && a != out && held && tripped && bits && maskCopy && bits != maskCopy && maskA != bits &&
           maskA != maskCopy && cbgn_shape_ok(C, G, H, W) && (relu == 0 || relu == 1) &&
           (dtype == CB_F32 || dtype == CB_F16) && (const void*)held != out && (const void*)tripped != out &&
           (const void*)bits != out && (const void*)maskCopy != out;
}

}  // namespace

int cbinfer_groupnorm_supported(int C, int G) { return C >= 1 && C <= CBGN_MAX_C && G >= 1 && C % G == 0; }

int cbinfer_groupnorm_partials(const void* a, double* partials, const uint64_t* maskA, const uint64_t* bits, int all,
                               int C, int H, int W, int dtype, cbStream_t stream) {
    CB_REQUIRE(cbgn_partials_ok(a, partials, maskA, bits, C, H, W, dtype));
    const int wpr = (W + 63) / 64, nblk = (C + CBGN_BLOCK - 1) / CBGN_BLOCK;
    const long words = (long)H * wpr;
    cb_dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((cbgn_partials_kernel<T>), dim3(cb_walk_grid(words * nblk)), dim3(256), 0,
                           (hipStream_t)stream, (const T*)a, partials, (const unsigned long long*)maskA,
                           (const unsigned long long*)bits, all != 0, words, nblk, C, H, W, wpr);
    });
    return cb_launch_status();
}

int cbinfer_groupnorm_stats(const double* partials, float* stats, float* held, int32_t* tripped, int C, int G, int H,
                            int W, const double* eps, float threshold, int all, cbStream_t stream) {
    CB_REQUIRE(cbgn_stats_ok(partials, stats, held, tripped, C, G, H, W, eps, threshold));
    const long words = (long)H * ((W + 63) / 64);
    const double n = (double)((long)(C / G) * H * W);
    hipLaunchKernelGGL(cbgn_stats_kernel, dim3(G), dim3(CBGN_STAT_THREADS), 0, (hipStream_t)stream, partials, stats, held,
                       (int*)tripped, words, C, G, n, *eps, threshold, all != 0);
    return cb_launch_status();
}

int cbinfer_groupnorm_changed(const void* a, void* out, const float* gamma, const float* beta, const float* held,
                              const int32_t* tripped, const uint64_t* maskA, int all, uint64_t* bits, uint64_t* maskCopy,
                              int C, int G, int H, int W, int relu, int dtype, cbStream_t stream) {
    CB_REQUIRE(cbgn_apply_ok(a, out, held, tripped, maskA, bits, maskCopy, C, G, H, W, relu, dtype));
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    cb_dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((cbgn_apply_kernel<T>), dim3(cb_walk_grid(words)), dim3(256), 0, (hipStream_t)stream,
                           (const T*)a, (T*)out, gamma, beta, held, (const int*)tripped,
                           (const unsigned long long*)maskA, all != 0, (unsigned long long*)bits,
                           (unsigned long long*)maskCopy, words, C, G, H, W, wpr, relu);
    });
    return cb_launch_status();
}

int cbinfer_cbgroupnorm_forward(const void* a, const float* gamma, const float* beta, void* outputState, double* partials,
                                float* stats, float* held, int32_t* tripped, const uint64_t* maskA, const int32_t* listA,
                                int capA, const int32_t* countA, uint64_t* bits, uint64_t* maskCopy, int C, int G, int H,
                                int W, const double* eps, int relu, float threshold, int all, int dtype,
                                cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(cbgn_partials_ok(a, partials, maskA, bits, C, H, W, dtype));
    CB_REQUIRE(cbgn_stats_ok(partials, stats, held, tripped, C, G, H, W, eps, threshold));
    CB_REQUIRE(cbgn_apply_ok(a, outputState, held, tripped, maskA, bits, maskCopy, C, G, H, W, relu, dtype));
    CB_REQUIRE(capA >= 0 && !(maskA && listA) && (listA || !countA) && (const void*)partials != outputState &&
               (const void*)stats != outputState);
    // (a fresh state is written completely: the operand's change information is not used)
    const int every = all || (!maskA && !listA);
    if (listA && !every) {
        const int st = cb_list_to_bits(listA, capA, countA, H, W, bits, stream);
        if (st != CB_OK) return st;
    }
    int st = cbinfer_groupnorm_partials(a, partials, every ? nullptr : maskA, bits, every, C, H, W, dtype, stream);
    if (st != CB_OK) return st;
    st = cbinfer_groupnorm_stats(partials, stats, held, tripped, C, G, H, W, eps, threshold, all, stream);
    if (st != CB_OK) return st;
    return cbinfer_groupnorm_changed(a, outputState, gamma, beta, held, tripped, every ? nullptr : maskA, every, bits,
                                     maskCopy, C, G, H, W, relu, dtype, stream);
}
