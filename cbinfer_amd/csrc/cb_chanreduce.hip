// Change-based reductions over the channel axis of one pixel -- channels-first LayerNorm, L2 normalisation, softmax and
// log-softmax -- on gfx950.  The reference has no such operator; contracts of the entry points in
// include/cbinfer_hip.h.  The output at a pixel depends on the C values at that pixel alone, and every producer of this
// library leaves the pixels outside its change list bit for bit as they were: recomputing at the operand's changed
// pixels gives the dense result exactly, without a threshold.  A frame is
//   for an operand in LIST form, one launch in front: the list's bits ORed into the zeroed working mask
//              (cb_list_to_bits of cb_maskwalk.h);
//   one launch, the word-level walk of cb_maskwalk.h (cb_walk_word_units): the unit of work is a non-empty mask word,
//              up to 64 pixels of a row, lane <-> pixel.
// The summation order is the specification's (sum16 / max16: 16 slices c mod 16, each in ascending c, combined in the
// fixed tree p[2i] op p[2i+1]) and does not depend on the launch: a word with more than 16 listed pixels gives a thread
// four slices of one pixel, a word with at most 16 gives it one, and both evaluate the same tree.  A thread's values are
// read from global memory once and held in its own LDS column over the passes (up to 48 KiB, sized by C per launch);
// beyond that every pass reads them again.  No data atomics, host sync, memset, allocation or inline assembly; all
// stores are plain vector stores.
#include "cb_maskwalk.h"

// hipcc contracts a * b + c to an FMA by default, so the arithmetic below is written with operators under this file's
// pragma: everything is evaluated as written, one rounding per operation (as cb_pointwise.hip).
#pragma clang fp contract(off)

namespace {

// What the LDS holds over the passes is decided per launch, by C alone, with 48 values per thread (48 KiB) at most:
//   CBR_HOLD_ALL   C <= 192: both forms hold their values (a thread of the four-slice form has 4 ceil(C / 16));
//   CBR_HOLD_FEW   C <= 768: only a word of at most 16 listed pixels does (ceil(C / 16) values per thread);
//   CBR_HOLD_NONE  beyond: every pass reads global memory again.
// The launch asks for what its C needs, 1 KiB per value (DESIGN 5.21 has the measurement).
enum { CBR_HOLD_NONE, CBR_HOLD_FEW, CBR_HOLD_ALL };
constexpr int CBR_HELD = 48;
inline int cbr_hold_mode(int C) {
    const long per = ((long)C + 15) / 16;
    return 4 * per <= CBR_HELD ? CBR_HOLD_ALL : per <= CBR_HELD ? CBR_HOLD_FEW : CBR_HOLD_NONE;
}
inline int cbr_held_values(int C) {
    const int per = (int)(((long)C + 15) / 16), mode = cbr_hold_mode(C);
    return mode == CBR_HOLD_ALL ? 4 * per : mode == CBR_HOLD_FEW ? per : 0;
}

// p[2i] op p[2i+1], level by level, of N = 1, 2, 4, 8 or 16 neighbouring nodes of the specification's tree
template <int N, bool MAX>
__device__ __forceinline__ float cbr_tree(float (&p)[N]) {
#pragma unroll
    for (int m = N; m > 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < m / 2; ++i) {
            const float a = p[2 * i], b = p[2 * i + 1];
            p[i] = MAX ? (b > a ? b : a) : a + b;
        }
    return p[0];
}

// The channels of one pixel as thread (pixel px of PX, slices s0 .. s0 + SL - 1) sees them, and the reductions over
// them.  SL = 4: PX = 64 pixels, wave k owns the slices 4k .. 4k + 3;  SL = 1: PX = 16 pixels, one slice per thread.
// HELD: the thread's values are loaded ONCE into its own column of `held` (LDS,
// [value][thread]: no other thread reads them, so no barrier is needed) and every pass reads those; otherwise every
// pass reads them again from global memory.  The values and the order of the operations are the same either way.
// `red` holds two regions of 256 floats, used in turn: a reduction's partials are read behind ONE barrier, and the
// region is written again only behind the barrier of the reduction after it.
template <typename T, int SL, bool HELD>
struct cbr_pixel {
    static constexpr int PX = SL == 4 ? 64 : 16, NP = 16 / SL;
    const T* xp;      // the pixel's value of channel 0
    long HW;
    int C, px, grp;
    bool live;        // this thread has a pixel
    float* red;
    unsigned& turn;
    float* held;      // this thread's column

    __device__ __forceinline__ void stage() const {
        if (!HELD || !live) return;
        float* h = held;
        for (int c0 = grp * SL; c0 < C; c0 += 16, h += SL * 256) {
#pragma unroll
            for (int j = 0; j < SL; ++j)
                if (c0 + j < C) h[j * 256] = cb_load_f32(xp + (long)(c0 + j) * HW);
        }
    }

    // f(j, c, x[c]) for the channels of the thread's slices, each slice in ascending c; j the slice's accumulator
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
        if (!live) return;
        const float* h = held;
        for (int c0 = grp * SL; c0 < C; c0 += 16, h += SL * 256) {
#pragma unroll
            for (int j = 0; j < SL; ++j)
                if (c0 + j < C) f(j, c0 + j, HELD ? h[j * 256] : cb_load_f32(xp + (long)(c0 + j) * HW));
        }
    }

    // sum16 / max16 of value(c, x[c]): on every thread of the pixel (uniform barriers: all 256 threads call this)
    template <bool MAX, typename V>
    __device__ __forceinline__ float reduce(V value) const {
        float a[SL];
#pragma unroll
        for (int j = 0; j < SL; ++j) a[j] = MAX ? -INFINITY : 0.f;
        each([&](int j, int c, float v) {
            const float t = value(c, v);
            a[j] = MAX ? (t > a[j] ? t : a[j]) : a[j] + t;
        });
        float* r = red + (turn++ & 1u) * 256;
        r[grp * PX + px] = cbr_tree<SL, MAX>(a);
        __syncthreads();
        float p[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) p[i] = r[i * PX + px];
        return cbr_tree<NP, MAX>(p);
    }
};

// One non-empty word.  All of the arithmetic is the specification's, in f32; the result is rounded to T once.
template <typename T, int KIND, int SL, bool HELD>
__device__ __forceinline__ void cbr_word(const T* __restrict__ x, T* __restrict__ out, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, float eps, unsigned long long word, int n,
                                         long first, long HW, int C, float* red, unsigned& turn, float* held) {
    constexpr int PX = SL == 4 ? 64 : 16;
    const int px = threadIdx.x & (PX - 1);
    const bool live = px < n;
    const int bit = n == 64 ? px : cb_select_bit(word, live ? px : 0);
    const cbr_pixel<T, SL, HELD> pix = {x + first + bit, HW, C, px, (int)threadIdx.x / PX, live, red, turn,
                                        held + threadIdx.x};
    pix.stage();
    T* op = out + first + bit;
    const float fC = (float)C;
    if (KIND == CB_CH_LAYERNORM) {
        const float mean = pix.template reduce<false>([](int, float v) { return v; }) / fC;
        const float var = pix.template reduce<false>([&](int, float v) {
            const float d = v - mean;
            return d * d;
        }) / fC;
        const float r = 1.f / sqrtf(var + eps);
        pix.each([&](int, int c, float v) {
            float y = (v - mean) * r;
            if (gamma) {
                y = y * gamma[c];
                y = y + beta[c];
            }
            op[(long)c * HW] = (T)y;
        });
    } else if (KIND == CB_CH_L2NORM) {
        const float t = sqrtf(pix.template reduce<false>([](int, float v) { return v * v; }));
        const float den = t < eps ? eps : t;
        pix.each([&](int, int c, float v) { op[(long)c * HW] = (T)(v / den); });
    } else {
        const float m = pix.template reduce<true>([](int, float v) { return v; });
        const float s = pix.template reduce<false>([&](int, float v) { return expf(v - m); });
        const float logs = KIND == CB_CH_LOGSOFTMAX ? logf(s) : 0.f;
        pix.each([&](int, int c, float v) {
            const float a = v - m;
            op[(long)c * HW] = (T)(KIND == CB_CH_LOGSOFTMAX ? a - logs : expf(a) / s);
        });
    }
}

// x, out [C, H, W].  mask: the operand's change mask of this frame, or NULL; all: every pixel is listed.  An operand
// without a mask has its bits in `bits` already (list form) -- or did not change.  gamma / beta [C] (both or neither,
// CB_CH_LAYERNORM only).
template <typename T, int KIND, int HOLD>
__global__ __launch_bounds__(256) void cbr_chanreduce_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                            const unsigned long long* __restrict__ mask, int all,
                                                            unsigned long long* bits,
                                                            unsigned long long* __restrict__ maskCopy,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, long words, int C,
                                                            int H, int W, int wpr) {
    __shared__ float red[2 * 256];
    extern __shared__ float held[];      // cbr_held_values(C) x 256
    const long HW = (long)H * W;
    unsigned turn = 0;
    cb_walk_word_units(
        bits, maskCopy, words, W, wpr, all, [&](long w, int, int) { return mask ? mask[w] : 0ull; },
        [&](unsigned long long word, int y, int tile) {
            const int n = __popcll(word);
            const long first = (long)y * W + tile * 64;      // (H W fits an int: cbr_args_ok)
            // (the word is uniform over the workgroup, and so are the barriers of either form)
            if (n > 16)
                cbr_word<T, KIND, 4, HOLD == CBR_HOLD_ALL>(x, out, gamma, beta, eps, word, n, first, HW, C, red, turn, held);
            else
                cbr_word<T, KIND, 1, HOLD != CBR_HOLD_NONE>(x, out, gamma, beta, eps, word, n, first, HW, C, red, turn,
                                                            held);
        });
}

template <typename T>
void cbr_launch(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits, uint64_t* maskCopy, int C, int H,
                int W, int kind, float eps, const float* gamma, const float* beta, hipStream_t s) {
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
    const int hold = cbr_hold_mode(C);
    const size_t lds = (size_t)cbr_held_values(C) * 1024;
#define CBR_GO(KIND, HOLD)                                                                                            \
    if (kind == KIND && hold == HOLD)                                                                                 \
    hipLaunchKernelGGL((cbr_chanreduce_kernel<T, KIND, HOLD>), grid, block, lds, s, (const T*)x, (T*)out,             \
                       (const unsigned long long*)mask, all, (unsigned long long*)bits, (unsigned long long*)maskCopy, \
                       gamma, beta, eps, words, C, H, W, wpr)
#define CBR_KIND(KIND)            \
    CBR_GO(KIND, CBR_HOLD_NONE);  \
    CBR_GO(KIND, CBR_HOLD_FEW);   \
    CBR_GO(KIND, CBR_HOLD_ALL)
    CBR_KIND(CB_CH_LAYERNORM);
    CBR_KIND(CB_CH_L2NORM);
    CBR_KIND(CB_CH_SOFTMAX);
    CBR_KIND(CB_CH_LOGSOFTMAX);
#undef CBR_KIND
#undef CBR_GO
}

// what both entry points ask of the tensors, the module's two masks and the function
bool cbr_args_ok(const void* x, const void* out, const uint64_t* mask, const uint64_t* bits, const uint64_t* maskCopy,
                 int C, int H, int W, int kind, float eps, const float* gamma, const float* beta, int dtype) {
    return x && out && x != out && bits && maskCopy && bits != maskCopy && mask != bits && mask != maskCopy && H >= 1 &&
           W >= 1 && (dtype == CB_F32 || dtype == CB_F16) && cbinfer_chanreduce_supported(kind, C, eps) &&
           !gamma == !beta && (!gamma || kind == CB_CH_LAYERNORM) &&
           // (a list addresses a pixel with an int32; 64 C as for the other mask-driven operators)
           (long)H * W < (1l << 31) && (long)C * 64 < (1l << 31);
}

}  // namespace

int cbinfer_chanreduce_supported(int kind, int C, float eps) {
    return kind >= CB_CH_LAYERNORM && kind <= CB_CH_LOGSOFTMAX && C >= 1 && eps >= 0.f;      // (a NaN eps is not >= 0)
}

int cbinfer_chanreduce_changed(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits, uint64_t* maskCopy,
                               int C, int H, int W, int kind, float eps, const float* gamma, const float* beta, int dtype,
                               cbStream_t stream) {
    CB_REQUIRE(cbr_args_ok(x, out, mask, bits, maskCopy, C, H, W, kind, eps, gamma, beta, dtype));
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbr_launch<decltype(t)>(x, out, mask, all, bits, maskCopy, C, H, W, kind, eps, gamma, beta, (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbchanreduce_forward(const void* x, void* outputState, const uint64_t* mask, const int32_t* list, int capN,
                                 const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int kind,
                                 float eps, const float* gamma, const float* beta, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(cbr_args_ok(x, outputState, mask, bits, maskCopy, C, H, W, kind, eps, gamma, beta, dtype));
    CB_REQUIRE(capN >= 0 && !(mask && list) && (list || !countDev));
    if (list) {
        const int st = cb_list_to_bits(list, capN, countDev, H, W, bits, stream);
        if (st != CB_OK) return st;
    }
    return cbinfer_chanreduce_changed(x, outputState, mask, !mask && !list, bits, maskCopy, C, H, W, kind, eps, gamma,
                                      beta, dtype, stream);
}
