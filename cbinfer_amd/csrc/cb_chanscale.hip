// Change-based channel attention scale, out[c, p] = a[c, p] * held[c], on gfx950: the excite of a
// squeeze-and-excitation block.  The reference has no such operator; contracts of the entry points and the arithmetic in
// include/cbinfer_hip.h.  The gate vector g(s) of a frame moves a little in every frame of a video, so the library's own
// rule is applied to it: a channel whose gate moved by no more than `threshold` keeps the gate it last used (`held`), and
// its plane is recomputed only at the operand's changed pixels; a channel whose gate moved by more -- it TRIPPED -- takes
// the new gate and its whole plane is recomputed.  A frame is
//   for an operand in LIST form, one launch in front: the list's bits ORed into the zeroed working mask
//              (cb_list_to_bits of cb_maskwalk.h);
//   launch 1   cbcs_gate_kernel, ONE workgroup: s (the frame's vector, or the two-layer excitation of the pooled vector,
//              summed in the order of sum16), gate = g(s), the trip decision per channel, `held` updated at the tripped
//              channels, the tripped channels as ballot words and their count;
//   launch 2   cbcs_apply_kernel, the word walk of cb_maskwalk.h (cb_walk_word_units): every channel at a listed pixel,
//              the tripped channels at every other pixel.
// Two launches, since the workgroups of launch 2 read `held` while a one-launch form would still be writing it.  No
// atomics, host sync, memset, allocation or inline assembly; all stores are plain vector stores.
#include "cb_maskwalk.h"

// every product and sum below is rounded on its own, in the order written (as cb_pointwise.hip)
#pragma clang fp contract(off)

namespace {

constexpr int CBCS_MAX_C = 4096, CBCS_MAX_R = 1024;

// gate = g(s), the formulas of CB_PW_SIGMOID / CB_PW_HARDSIGMOID (comparisons: a NaN stays a NaN)
__device__ __forceinline__ float cbcs_gate(float s, int gateFn) {
    if (gateFn == CB_CS_GATE_SIGMOID) return 1.f / (1.f + expf(-s));
    if (gateFn == CB_CS_GATE_HARDSIGMOID) {
        const float t = s + 3.f;
        return (t < 0.f ? 0.f : (t > 6.f ? 6.f : t)) / 6.f;
    }
    return s;
}

__device__ __forceinline__ float cbcs_act(float v, int act) {
    if (act == CB_CS_ACT_SILU) return v / (1.f + expf(-v));
    return v < 0.f ? 0.f : v;      // CB_CS_ACT_RELU (-0 and a NaN stay)
}

// (T)(x * h): the f32 product rounded to f32, then rounded to T.  Written as (T)(x * h) alone, hipcc forms the f16 result
// as ONE v_fma_mixlo_f16 with an addend of +0: the product is then rounded once from its exact value -- not the
// specification's two roundings -- and a zero product loses its sign.  Under strict exception semantics both operations
// stay the instructions they are written as.
template <typename T>
__device__ __forceinline__ T cbcs_scaled(float x, float h) {
#pragma clang fp exceptions(strict)
    const float p = x * h;
    return (T)p;
}

// sum16 over k < n of w[k] * x[k] on the 16 lanes of one row: lane l owns the slice k = l mod 16 in ascending k, then
// the fixed tree p[2i] + p[2i+1] as a butterfly (an IEEE sum does not depend on the order of its two operands, so
// every lane ends with the tree's value).  All 64 lanes of the wave are active; `live` rows only read memory.
__device__ __forceinline__ float cbcs_row_sum16(const float* __restrict__ w, const float* x, int n, int lane, bool live) {
    float p = 0.f;
    if (live)
        for (int k = lane; k < n; k += 16) p = p + w[k] * x[k];
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) p = p + __shfl_xor(p, m, 16);
    return p;
}

// One workgroup of 256 threads.  v [C] (T): the frame's vector, or -- w1 != NULL -- the pooled vector z of the
// excitation hidden = act(W1 z + b1), s = W2 hidden + b2 (W1 [R, C], W2 [C, R], b1 / b2 f32 or NULL).  gate, held [C]
// f32; tripped ceil(C / 64) words, every one written; tripCount one int.
template <typename T>
__global__ __launch_bounds__(256) void cbcs_gate_kernel(const T* __restrict__ v, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, float* __restrict__ gate,
                                                       float* __restrict__ held,
                                                       unsigned long long* __restrict__ tripped,
                                                       int* __restrict__ tripCount, int C, int R, int gateFn, int act,
                                                       float threshold, int all) {
    __shared__ float vec[CBCS_MAX_C];      // z, then s
    __shared__ float hidden[CBCS_MAX_R];
    __shared__ int counts[4];
    const int tid = threadIdx.x, lane16 = tid & 15, row = tid >> 4;
    for (int c = tid; c < C; c += 256) vec[c] = cb_load_f32(v + c);
    __syncthreads();
    if (w1) {
        // (the bounds of both loops are uniform over the workgroup: every lane takes part in every butterfly)
        for (int r0 = 0; r0 < R; r0 += 16) {
            const int r = r0 + row;
            const bool live = r < R;
            float h = cbcs_row_sum16(w1 + (long)(live ? r : 0) * C, vec, C, lane16, live);
            if (live && lane16 == 0) {
                if (b1) h = h + b1[r];
                hidden[r] = cbcs_act(h, act);
            }
        }
        __syncthreads();      // hidden is complete, and z has been read for the last time
        for (int c0 = 0; c0 < C; c0 += 16) {
            const int c = c0 + row;
            const bool live = c < C;
            float s = cbcs_row_sum16(w2 + (long)(live ? c : 0) * R, hidden, R, lane16, live);
            if (live && lane16 == 0) {
                if (b2) s = s + b2[c];
                vec[c] = s;
            }
        }
        __syncthreads();
    }
    // 256 channels per round, one ballot word per wave; the rounds are uniform, the predicate carries the bound
    const int wave = tid >> 6, nwords = (C + 63) / 64;
    int mine = 0;
    for (int base = 0; base < nwords * 64; base += 256) {
        const int c = base + tid;
        bool trip = false;
        if (c < C) {
            const float g = cbcs_gate(vec[c], gateFn);
            gate[c] = g;
            // strictly more than the threshold; a NaN trips
            trip = all || !(fabsf(g - held[c]) <= threshold);
            if (trip) held[c] = g;
        }
        const unsigned long long word = __ballot(trip);
        const int j = base / 64 + wave;
        if (j < nwords) {
            if ((tid & 63) == 0) tripped[j] = word;
            mine += __popcll(word);
        }
    }
    if ((tid & 63) == 0) counts[wave] = mine;
    __syncthreads();
    if (tid == 0) *tripCount = counts[0] + counts[1] + counts[2] + counts[3];
}

// a, out [C, H, W]; held [C] f32; tripped / tripCount as launch 1 left them.  maskA: the operand's change mask of this
// frame, or NULL; all: every pixel is listed with every channel.  An operand without a mask has its bits in `bits`
// already (list form) -- or did not change.  In a frame with tripped channels the frame's mask is the full row word; a
// pixel that is not listed is written in the tripped channels only.
template <typename T>
__global__ __launch_bounds__(256) void cbcs_apply_kernel(const T* __restrict__ a, T* __restrict__ out,
                                                        const float* __restrict__ held,
                                                        const unsigned long long* __restrict__ tripped,
                                                        const int* __restrict__ tripCount,
                                                        const unsigned long long* __restrict__ maskA, int all,
                                                        unsigned long long* bits,
                                                        unsigned long long* __restrict__ maskCopy, long words, int C,
                                                        int H, int W, int wpr) {
    __shared__ unsigned short chans[CBCS_MAX_C];      // the tripped channels, ascending
    const long HW = (long)H * W;
    const int full = all || *tripCount > 0;      // (uniform over the launch: the frame's mask is the full row word)
    int n = 0;
    if (full && !all) {
        // The list is made from the words alone, cut to the C channels, and n counted from them: whatever the buffers
        // hold, every entry is a channel of the map and the list has n of them.
        const int nwords = (C + 63) / 64, lane = threadIdx.x & 63;
        const unsigned long long last = (C & 63) ? ((1ull << (C & 63)) - 1ull) : ~0ull;
        auto wordOf = [&](int i) { return i == nwords - 1 ? (tripped[i] & last) : tripped[i]; };
        for (int j = threadIdx.x >> 6; j < nwords; j += 4) {
            int before = 0;
            for (int i = 0; i < j; ++i) before += __popcll(wordOf(i));
            const unsigned long long word = wordOf(j);
            if ((word >> lane) & 1ull) chans[before + __popcll(word & ((1ull << lane) - 1ull))] = j * 64 + lane;
        }
        for (int i = 0; i < nwords; ++i) n += __popcll(wordOf(i));
        __syncthreads();
    }
    unsigned long long listed = 0;
    cb_walk_word_units(
        bits, maskCopy, words, W, wpr, full,
        // (the working word is zeroed only behind the barrier that follows the unit)
        [&](long w, int, int) { return listed = bits[w] | (maskA ? maskA[w] : 0ull); },
        [&](unsigned long long word, int y, int tile) {
            const long first = (long)y * W + tile * 64;      // (H W fits an int: cbcs_apply_ok)
            const unsigned long long every = all ? word : (listed & word);
            cb_walk_items(every, C, [&](int c, int bit) {
                const long o = (long)c * HW + first + bit;
                out[o] = cbcs_scaled<T>(cb_load_f32(a + o), held[c]);
            });
            cb_walk_items(word & ~every, n, [&](int i, int bit) {
                const int c = chans[i];
                const long o = (long)c * HW + first + bit;
                out[o] = cbcs_scaled<T>(cb_load_f32(a + o), held[c]);
            });
        });
}

bool cbcs_gate_ok(const void* v, const float* w1, const float* b1, const float* w2, const float* b2, const float* gate,
                  const float* held, const uint64_t* tripped, const int32_t* tripCount, int C, int R, int gateFn, int act,
                  float threshold, int dtype) {
    return v && gate && held && tripped && tripCount && gate != held && (const void*)gate != v &&
           (const void*)held != v && (dtype == CB_F32 || dtype == CB_F16) &&
           cbinfer_chanscale_supported(gateFn, act, C, R) && threshold >= 0.f &&      // (a NaN threshold is not >= 0)
           (R > 0 ? (w1 && w2) : (!w1 && !w2 && !b1 && !b2));
}

bool cbcs_apply_ok(const void* a, const void* out, const float* held, const uint64_t* tripped, const int32_t* tripCount,
                   const uint64_t* maskA, const uint64_t* bits, const uint64_t* maskCopy, int C, int H, int W,
                   int dtype) {
    return a && out && a != out && held && tripped && tripCount && bits && maskCopy && bits != maskCopy &&
           maskA != bits && maskA != maskCopy && C >= 1 && C <= CBCS_MAX_C && H >= 1 && W >= 1 &&
           (dtype == CB_F32 || dtype == CB_F16) && (const void*)held != out && (const void*)tripped != out &&
           // (a list addresses a pixel with an int32)
           (long)H * W < (1l << 31);
}

}  // namespace

int cbinfer_chanscale_supported(int gate, int act, int C, int R) {
    if (gate < CB_CS_GATE_NONE || gate > CB_CS_GATE_HARDSIGMOID) return 0;
    if (C < 1 || C > CBCS_MAX_C || R < 0 || R > CBCS_MAX_R) return 0;
    // (the excitation has an activation, the plain form has none)
    return R > 0 ? (act == CB_CS_ACT_RELU || act == CB_CS_ACT_SILU) : act == CB_CS_ACT_NONE;
}

int cbinfer_chanscale_gate(const void* v, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                           float* held, uint64_t* tripped, int32_t* tripCount, int C, int R, int gateFn, int act,
                           float threshold, int all, int dtype, cbStream_t stream) {
    CB_REQUIRE(cbcs_gate_ok(v, w1, b1, w2, b2, gate, held, tripped, tripCount, C, R, gateFn, act, threshold, dtype));
    cb_dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((cbcs_gate_kernel<T>), dim3(1), dim3(256), 0, (hipStream_t)stream, (const T*)v, w1, b1, w2, b2,
                           gate, held, (unsigned long long*)tripped, (int*)tripCount, C, R, gateFn, act, threshold,
                           all != 0);
    });
    return cb_launch_status();
}

int cbinfer_chanscale_changed(const void* a, void* out, const float* held, const uint64_t* tripped,
                              const int32_t* tripCount, const uint64_t* maskA, int all, uint64_t* bits, uint64_t* maskCopy,
                              int C, int H, int W, int dtype, cbStream_t stream) {
    CB_REQUIRE(cbcs_apply_ok(a, out, held, tripped, tripCount, maskA, bits, maskCopy, C, H, W, dtype));
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    cb_dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((cbcs_apply_kernel<T>), dim3(cb_walk_grid(words)), dim3(256), 0, (hipStream_t)stream,
                           (const T*)a, (T*)out, held, (const unsigned long long*)tripped, (const int*)tripCount,
                           (const unsigned long long*)maskA, all != 0, (unsigned long long*)bits,
                           (unsigned long long*)maskCopy, words, C, H, W, wpr);
    });
    return cb_launch_status();
}

int cbinfer_cbchanscale_forward(const void* a, const void* v, const float* w1, const float* b1, const float* w2,
                                const float* b2, void* outputState, float* gate, float* held, uint64_t* tripped,
                                int32_t* tripCount, const uint64_t* maskA, const int32_t* listA, int capA,
                                const int32_t* countA, uint64_t* bits, uint64_t* maskCopy, int C, int R, int H, int W,
                                int gateFn, int act, float threshold, int all, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(cbcs_gate_ok(v, w1, b1, w2, b2, gate, held, tripped, tripCount, C, R, gateFn, act, threshold, dtype));
    CB_REQUIRE(cbcs_apply_ok(a, outputState, held, tripped, tripCount, maskA, bits, maskCopy, C, H, W, dtype));
    CB_REQUIRE(capA >= 0 && !(maskA && listA) && (listA || !countA) && v != outputState && v != a);
    // (a fresh state is written completely: the operand's change information is not used)
    const int every = all || (!maskA && !listA);
    if (listA && !every) {
        const int st = cb_list_to_bits(listA, capA, countA, H, W, bits, stream);
        if (st != CB_OK) return st;
    }
    const int st = cbinfer_chanscale_gate(v, w1, b1, w2, b2, gate, held, tripped, tripCount, C, R, gateFn, act, threshold,
                                          all, dtype, stream);
    if (st != CB_OK) return st;
    return cbinfer_chanscale_changed(a, outputState, held, tripped, tripCount, every ? nullptr : maskA, every, bits,
                                     maskCopy, C, H, W, dtype, stream);
}
