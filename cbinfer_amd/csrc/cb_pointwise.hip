// Change-based element-wise function of one map, out = act(x scale[c] + shift[c]), on gfx950.  The
// reference has no such operator; contracts of the entry points in include/cbinfer_hip.h.  Every producer of this library
// leaves the pixels outside its change list bit for bit as they were, so f(x) can differ from last frame's only at the
// operand's changed pixels: recomputing there gives the dense result exactly, without a threshold.  A frame is
//   for an operand in LIST form, one launch in front: the list's bits ORed into the zeroed working mask
//              (cb_list_to_bits of cb_maskwalk.h);
//   one launch, the word walk of cb_maskwalk.h (cb_walk_words): the operand's change mask (or the full row word of an
//              operand without change information) is ORed into the working word, one value per (set bit, channel).
// The function is a template parameter (one kernel per kind and dtype); the affine and its per-channel operands are
// decided by a pointer that is uniform over the launch.  No LDS, host sync, memset, allocation, data atomics or inline
// assembly.
#include "cb_maskwalk.h"

// hipcc contracts a * b + c to an FMA by default -- also through __fmul_rn / __fadd_rn, which are plain operators compiled
// under the header's own setting --, so the arithmetic below is written with operators under this file's pragma:
// everything is evaluated as written, one rounding per operation.
#pragma clang fp contract(off)

namespace {

// lo <= t <= hi by comparisons: a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float cbw_clamp(float t, float lo, float hi) { return t < lo ? lo : (t > hi ? hi : t); }

// One value, all in f32; every operation is a correctly rounded IEEE one in the order written (nothing is contracted to
// an FMA), so a float32 twin on the host reproduces the bits of the seven kinds without a transcendental function.
template <int KIND>
__device__ __forceinline__ float cbw_act(float v, float p0, float p1, float slope) {
    switch (KIND) {
        case CB_PW_RELU: return v < 0.f ? 0.f : v;      // (-0 and a NaN stay, as torch.relu)
        case CB_PW_HARDTANH: return cbw_clamp(v, p0, p1);
        case CB_PW_LEAKY: return v > 0.f ? v : v * p0;
        case CB_PW_PRELU: return v > 0.f ? v : slope * v;
        case CB_PW_HARDSWISH: return v * cbw_clamp(v + 3.f, 0.f, 6.f) / 6.f;
        case CB_PW_HARDSIGMOID: return cbw_clamp(v + 3.f, 0.f, 6.f) / 6.f;
        case CB_PW_SIGMOID: return 1.f / (1.f + expf(-v));
        case CB_PW_SILU: return v / (1.f + expf(-v));
        case CB_PW_TANH: return tanhf(v);
        // the six kinds of DESIGN 5.30: the device's erff / tanhf / expm1f / expf / log1pf, each bounded there
        case CB_PW_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
        case CB_PW_GELU_TANH:
            return 0.5f * v * (1.f + tanhf(0.79788456080286535588f * (v + 0.044715f * (v * v * v))));
        case CB_PW_ELU: return v > 0.f ? v : p0 * expm1f(v * p1);      // (CELU: p1 = 1 / alpha)
        case CB_PW_SELU: return v > 0.f ? 1.0507009873554805f * v : 1.7580993408473766f * expm1f(v);
        case CB_PW_SOFTPLUS: {
            const float t = v * p0;
            return t > p1 ? v : log1pf(expf(t)) / p0;
        }
        case CB_PW_MISH: return v * tanhf(log1pf(expf(v)));
        default: return v;      // CB_PW_IDENTITY: the affine alone
    }
}

// x, out [C, H, W].  mask: the operand's change mask of this frame, or NULL; all: every pixel is listed.  An operand
// without a mask has its bits in `bits` already (list form) -- or did not change.  scale / shift [C] (both or neither),
// slope [C] (CB_PW_PRELU only).
template <typename T, int KIND>
__global__ __launch_bounds__(256) void cbw_pointwise_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                           const unsigned long long* __restrict__ mask, int all,
                                                           unsigned long long* bits,
                                                           unsigned long long* __restrict__ maskCopy,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ slope, float p0, float p1,
                                                           long words, int C, int H, int W, int wpr) {
    const long HW = (long)H * W;
    cb_walk_words(
        bits, maskCopy, words, C, W, wpr, all, [&](long w, int, int) { return mask ? mask[w] : 0ull; },
        [&](int c, int y, int col) {
            const long o = (long)c * HW + (y * W + col);      // (H W fits an int: cbw_args_ok)
            float v = cb_load_f32(x + o);
            // two roundings, never one FMA
            if (scale) v = v * scale[c] + shift[c];
            v = cbw_act<KIND>(v, p0, p1, KIND == CB_PW_PRELU ? slope[c] : 0.f);
            out[o] = (T)v;      // fp16: rounded once
        });
}

template <typename T>
void cbw_launch(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits, uint64_t* maskCopy, int C, int H,
                int W, int kind, float p0, float p1, const float* scale, const float* shift, const float* slope,
                hipStream_t s) {
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBW_GO(KIND)                                                                                                  \
    case KIND:                                                                                                        \
        hipLaunchKernelGGL((cbw_pointwise_kernel<T, KIND>), grid, block, 0, s, (const T*)x, (T*)out,                  \
                           (const unsigned long long*)mask, all, (unsigned long long*)bits,                          \
                           (unsigned long long*)maskCopy, scale, shift, slope, p0, p1, words, C, H, W, wpr);         \
        break
    switch (kind) {
        CBW_GO(CB_PW_IDENTITY);
        CBW_GO(CB_PW_RELU);
        CBW_GO(CB_PW_HARDTANH);
        CBW_GO(CB_PW_LEAKY);
        CBW_GO(CB_PW_PRELU);
        CBW_GO(CB_PW_HARDSWISH);
        CBW_GO(CB_PW_HARDSIGMOID);
        CBW_GO(CB_PW_SIGMOID);
        CBW_GO(CB_PW_SILU);
        CBW_GO(CB_PW_TANH);
        CBW_GO(CB_PW_GELU);
        CBW_GO(CB_PW_GELU_TANH);
        CBW_GO(CB_PW_ELU);
        CBW_GO(CB_PW_SELU);
        CBW_GO(CB_PW_SOFTPLUS);
        CBW_GO(CB_PW_MISH);
    }
#undef CBW_GO
}

// what both entry points ask of the tensors, the module's two masks and the function
bool cbw_args_ok(const void* x, const void* out, const uint64_t* mask, const uint64_t* bits, const uint64_t* maskCopy,
                 int C, int H, int W, int kind, float p0, float p1, const float* scale, const float* shift,
                 const float* slope, int dtype) {
    return x && out && x != out && bits && maskCopy && bits != maskCopy && mask != bits && mask != maskCopy && C >= 1 &&
           H >= 1 && W >= 1 && (dtype == CB_F32 || dtype == CB_F16) && cbinfer_pointwise_supported(kind, p0, p1) &&
           (kind != CB_PW_PRELU || slope) && !scale == !shift &&
           // (a list addresses a pixel with an int32; the kernel numbers a word's items with an int)
           (long)H * W < (1l << 31) && (long)C * 64 < (1l << 31);
}

}  // namespace

int cbinfer_pointwise_supported(int kind, float p0, float p1) {
    // (10..15 are unassigned)
    if (!(kind >= CB_PW_IDENTITY && kind <= CB_PW_TANH) && !(kind >= CB_PW_GELU && kind <= CB_PW_MISH)) return 0;
    if (kind == CB_PW_HARDTANH && !(p0 <= p1)) return 0;      // (also a NaN bound)
    // finite: t - t == 0 fails for an infinity and a NaN
    if (kind == CB_PW_ELU && !(p0 - p0 == 0.f && p1 - p1 == 0.f)) return 0;
    if (kind == CB_PW_SOFTPLUS && (!(p0 - p0 == 0.f) || p0 == 0.f || p1 != p1)) return 0;
    return 1;
}

int cbinfer_pointwise_changed(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits, uint64_t* maskCopy,
                              int C, int H, int W, int kind, float p0, float p1, const float* scale, const float* shift,
                              const float* slope, int dtype, cbStream_t stream) {
    CB_REQUIRE(cbw_args_ok(x, out, mask, bits, maskCopy, C, H, W, kind, p0, p1, scale, shift, slope, dtype));
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbw_launch<decltype(t)>(x, out, mask, all, bits, maskCopy, C, H, W, kind, p0, p1, scale, shift, slope,
                                (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbpointwise_forward(const void* x, void* outputState, const uint64_t* mask, const int32_t* list, int capN,
                                const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int kind,
                                float p0, float p1, const float* scale, const float* shift, const float* slope, int dtype,
                                cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(cbw_args_ok(x, outputState, mask, bits, maskCopy, C, H, W, kind, p0, p1, scale, shift, slope, dtype));
    CB_REQUIRE(capN >= 0 && !(mask && list) && (list || !countDev));
    if (list) {
        const int st = cb_list_to_bits(list, capN, countDev, H, W, bits, stream);
        if (st != CB_OK) return st;
    }
    return cbinfer_pointwise_changed(x, outputState, mask, !mask && !list, bits, maskCopy, C, H, W, kind, p0, p1, scale,
                                     shift, slope, dtype, stream);
}
