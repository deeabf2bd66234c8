// Change-based depthwise convolution (groups == in_channels, channel multiplier) on gfx950.  The
// reference has no such operator; contracts of the entry points in include/cbinfer_hip.h.  A depthwise layer is not a
// contraction: output channel k reads input channel k / mult only, kH kW taps each.  It is a VALU stencil driven by the
// change mask of the OUTPUT map.  Not the word walk of cb_maskwalk.h (its unit is word x channel block and it only reads
// the mask copy); it takes the header's grid sizing, load pair and dtype dispatch:
//   unit       one mask word (64 consecutive output pixels of a row) x a block of 16 output channels; a persistent
//              grid strides over the units.  Lane = output column, unlisted lanes are predicated off, an empty word
//              costs its one load.  A wave takes four channels side by side (four independent loads per tap); the
//              channel index is wave-uniform, so filter and bias arrive by scalar loads and the row tests are
//              branches of the whole wave.
//   value      f32, ONE fixed order: bias (0 without one), then one FMA per in-map tap, ky outer, kx inner; rounded to
//              f16 once.  A pixel's bits depend neither on the other listed pixels nor on the launch form.
//   masks      frame-mask form: the units of channel block 0 copy the frame's mask and zero the other one, every
//              workgroup arrives once, the last flips the parity (cbinfer_conv_changed_tconv's protocol).
//              bits / maskCopy form: a launch in front moves `bits` to maskCopy and zeroes it (cbdw_take_kernel); the
//              stencil launch then only READS maskCopy -- with units that split a word's channels over workgroups no
//              unit could zero the word while others still read it.
// No LDS, no inline assembly, no atomics beyond the one arrival counter; all stores are plain vector stores.
#include "cb_maskwalk.h"

namespace {

#define CBDW_CB 16      // output channels per unit
#define CBDW_WC 4       // ... of which each of the four waves takes four, side by side

// bits -> maskCopy, bits <- 0 (all != 0: every pixel of the map is listed instead; bits is zeroed all the same)
__global__ __launch_bounds__(256) void cbdw_take_kernel(unsigned long long* __restrict__ bits,
                                                       unsigned long long* __restrict__ maskCopy, long words, int Wo,
                                                       int wpr, int all) {
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    const int tile = (int)(w % wpr);
    const unsigned long long m = all ? cb_valid_mask(Wo, tile) : bits[w];
    maskCopy[w] = m;
    bits[w] = 0ull;
}

// in [C, Hi, Wi], wgt [K, 1, kH, kW], out [K, Ho, Wo], K = C mult.  frameMasks: the frame mask buffer (mask form), or
// NULL and `mask` the read-only mask of the frame (bits form).
template <typename T, int ACT>
__global__ __launch_bounds__(256) void cbdw_kernel(const T* __restrict__ in, const T* __restrict__ wgt,
                                                  const T* __restrict__ bias, T* __restrict__ out,
                                                  unsigned long long* frameMasks,
                                                  const unsigned long long* __restrict__ mask, long words, int K,
                                                  int mult, int Hi, int Wi, int Ho, int Wo, int wpr, cbGeom g) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long HWi = (long)Hi * Wi, HWo = (long)Ho * Wo;
    const int taps = g.kH * g.kW;
    const int cblocks = (K + CBDW_CB - 1) / CBDW_CB;
    const unsigned long long* cur = mask;
    unsigned long long *other = nullptr, *copy = nullptr;
    int par = 0;
    if (frameMasks) {
        par = __hip_atomic_load((int*)(frameMasks + 2 * words), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cur = frameMasks + (par ? words : 0);
        other = frameMasks + (par ? 0 : words);
        copy = frameMasks + 2 * words + 2;
    }
    const long units = words * cblocks;
    for (long u = blockIdx.x; u < units; u += gridDim.x) {
        const int cb = (int)(u / words);
        const long w = u - (long)cb * words;
        const unsigned long long word = cur[w];      // (uniform over the workgroup)
        if (frameMasks && cb == 0 && threadIdx.x == 0) {
            copy[w] = word;
            other[w] = 0ull;
        }
        if (word == 0) continue;
        const int oy = (int)(w / wpr), ox = (int)(w - (long)oy * wpr) * 64 + lane;
        const bool listed = ((word >> lane) & 1ull) != 0 && ox < Wo;      // (a bit of the row padding is never computed)
        const int y0 = oy * g.sH - g.pH, x0 = ox * g.sW - g.pW;
        // the wave's four channels side by side: their loads are independent and unconditional (a lane that is not
        // listed, or whose tap lies left or right of the map, reads the row's first pixel and drops it), so four are in
        // flight per tap; each channel's sum keeps its own fixed order
        const int k0 = __builtin_amdgcn_readfirstlane(cb * CBDW_CB + wave * CBDW_WC);
        if (k0 >= K) continue;      // (uniform over the wave; no barrier inside the loop)
        const T *src[CBDW_WC], *wk[CBDW_WC];
        float acc[CBDW_WC];
#pragma unroll
        for (int j = 0; j < CBDW_WC; ++j) {
            const int k = min(k0 + j, K - 1);      // (a channel behind the last one is computed twice and not stored)
            src[j] = in + (long)(k / mult) * HWi;
            wk[j] = wgt + (long)k * taps;
            acc[j] = bias ? cb_load_f32(bias + k) : 0.f;
        }
        bool hit = false;
        for (int ky = 0; ky < g.kH; ++ky) {
            const int y = y0 + ky * g.dH;
            if ((unsigned)y >= (unsigned)Hi) continue;      // (uniform over the wave)
            const long rowOff = (long)y * Wi;
            for (int kx = 0; kx < g.kW; ++kx) {
                const int x = x0 + kx * g.dW;
                const bool ok = listed && (unsigned)x < (unsigned)Wi;
                const long off = rowOff + (ok ? x : 0);
                float v[CBDW_WC], wv[CBDW_WC];
#pragma unroll
                for (int j = 0; j < CBDW_WC; ++j) {
                    v[j] = cb_load_f32(src[j] + off);
                    wv[j] = cb_load_f32(wk[j] + ky * g.kW + kx);
                }
#pragma unroll
                for (int j = 0; j < CBDW_WC; ++j) acc[j] = ok ? __builtin_fmaf(wv[j], v[j], acc[j]) : acc[j];
                hit |= ok;
            }
        }
#pragma unroll
        for (int j = 0; j < CBDW_WC; ++j) {
            float r = acc[j];
            if (ACT >= CB_ACT_RELU) r = r != r ? r : (r > 0.f ? r : 0.f);      // (a NaN stays a NaN)
            if (ACT == CB_ACT_RELU6) r = r != r ? r : (r < 6.f ? r : 6.f);
            // (a pixel no tap reaches is never written)
            if (hit && k0 + j < K) out[(long)(k0 + j) * HWo + (long)oy * Wo + ox] = (T)r;
        }
    }
    // this workgroup has read the parity and its words
    if (frameMasks) cb_flip_parity_last((int*)(frameMasks + 2 * words), par, (int)gridDim.x);
}

template <typename T>
void cbdw_launch(const void* in, const void* wgt, const void* bias, void* out, uint64_t* frameMasks, const uint64_t* mask,
                 int K, int mult, int Hi, int Wi, int Ho, int Wo, const cbGeom& g, int act, hipStream_t s) {
    const int wpr = (Wo + 63) / 64;
    const long words = (long)Ho * wpr;
    const dim3 grid(cb_walk_grid(words * ((K + CBDW_CB - 1) / CBDW_CB))), block(256);
#define CBDW_GO(ACT)                                                                                                  \
    hipLaunchKernelGGL((cbdw_kernel<T, ACT>), grid, block, 0, s, (const T*)in, (const T*)wgt, (const T*)bias, (T*)out, \
                       (unsigned long long*)frameMasks, (const unsigned long long*)mask, words, K, mult, Hi, Wi, Ho,  \
                       Wo, wpr, g)
    if (act == CB_ACT_RELU6)
        CBDW_GO(CB_ACT_RELU6);
    else if (act == CB_ACT_RELU)
        CBDW_GO(CB_ACT_RELU);
    else
        CBDW_GO(CB_ACT_NONE);
#undef CBDW_GO
}

// the launch in front of a bits / maskCopy frame (cbdw_take_kernel), then the stencil reading maskCopy
int cbdw_take_and_launch(const void* in, const void* wgt, const void* bias, void* out, uint64_t* bits, uint64_t* maskCopy,
                         int all, int K, int mult, int Hi, int Wi, int Ho, int Wo, const cbGeom& g, int act, int dtype,
                         hipStream_t s) {
    const int wpr = (Wo + 63) / 64;
    const long words = (long)Ho * wpr;
    hipLaunchKernelGGL(cbdw_take_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s,
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, Wo, wpr, all);
    const int st = cb_launch_status();
    if (st != CB_OK) return st;
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbdw_launch<decltype(t)>(in, wgt, bias, out, nullptr, maskCopy, K, mult, Hi, Wi, Ho, Wo, g, act, s);
    });
    return cb_launch_status();
}

// CB_OK and the output map, or the status every entry point returns before its first launch
int cbdw_shape(int C, int mult, int Hi, int Wi, const cbGeom* geom, int act, int dtype, int* Ho, int* Wo) {
    CB_REQUIRE(geom && C > 0 && mult > 0 && Hi > 0 && Wi > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(act >= CB_ACT_NONE && act <= CB_ACT_RELU6);
    const int st = cbinfer_geom_out_size(Hi, Wi, geom, Ho, Wo);
    if (st != CB_OK) return st;
    CB_REQUIRE((long)C * mult < (1l << 31) / 64);
    const long K = (long)C * mult;
    // (the int32 guards of cbinfer_conv_changed_geom)
    if ((long)*Ho * *Wo >= (1l << 31) / K || (long)C * Hi * Wi * 4 >= (1l << 30)) return CB_ERR_UNSUPPORTED;
    return CB_OK;
}

// the pool window whose footprint is the filter's, or false: dilation 1 and p <= k / 2 per axis
bool cbdw_window(const cbGeom& g, cbPool* win) {
    const cbPool p = {g.kH, g.kW, g.sH, g.sW, g.pH, g.pW, 0, CB_POOL_MAX};
    *win = p;
    return g.dH == 1 && g.dW == 1 && cbinfer_pool_supported(&p);
}

}  // namespace

extern "C" {

int cbinfer_dwconv_supported(int C, int mult, const cbGeom* geom) {
    int Ho, Wo;
    if (!geom || C < 1 || mult < 1 || (long)C * mult >= (1l << 31) / 64) return 0;
    // (a map large enough for every filter within the limits: only the geometry is judged)
    return cbinfer_geom_out_size(64, 64, geom, &Ho, &Wo) == CB_OK;
}

int cbinfer_dwconv_changed(const void* input, const void* weight, const void* bias, void* output, uint64_t* frameMasks,
                           uint64_t* bits, uint64_t* maskCopy, int C, int mult, int Hi, int Wi, const cbGeom* geom,
                           int act, int dtype, cbStream_t stream) {
    CB_REQUIRE(input && weight && output);
    CB_REQUIRE(frameMasks ? (!bits && !maskCopy) : (bits && maskCopy && bits != maskCopy));
    int Ho, Wo;
    const int st = cbdw_shape(C, mult, Hi, Wi, geom, act, dtype, &Ho, &Wo);
    if (st != CB_OK) return st;
    if (!frameMasks)
        return cbdw_take_and_launch(input, weight, bias, output, bits, maskCopy, 0, C * mult, mult, Hi, Wi, Ho, Wo, *geom,
                                    act, dtype, (hipStream_t)stream);
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbdw_launch<decltype(t)>(input, weight, bias, output, frameMasks, nullptr, C * mult, mult, Hi, Wi, Ho, Wo, *geom,
                                 act, (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbdwconv2d_forward(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                               const void* weight, const void* bias, int C, int mult, int Hi, int Wi, const cbGeom* geom,
                               float threshold, int feedbackLoop, int copyInput, int act, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && prevInput && prevOutput && frameMasks && weight);
    int Ho, Wo;
    int st = cbdw_shape(C, mult, Hi, Wi, geom, act, dtype, &Ho, &Wo);
    if (st != CB_OK) return st;
    if (Hi > 65535) return CB_ERR_UNSUPPORTED;      // (cbinfer_change_detection_geom: one grid row per input row)
    const void* src = (feedbackLoop || copyInput) ? prevInput : input;
    const bool copyAll = !feedbackLoop && copyInput && prevInput != input;
    st = cbinfer_change_detection_geom(input, prevInput, frameMasks, C, Hi, Wi, geom, threshold,
                                       feedbackLoop ? 1 : (copyAll ? 2 : 0), dtype, stream);
    if (st != CB_OK) return st;
    return cbinfer_dwconv_changed(src, weight, bias, prevOutput, frameMasks, nullptr, nullptr, C, mult, Hi, Wi, geom, act,
                                  dtype, stream);
}

int cbinfer_cbdwconv2d_forward_propagated(const void* input, void* outputState, const int32_t* changeIndexes, int capN,
                                          const int32_t* countDev, const uint64_t* inputMask, int allPixels,
                                          uint64_t* bits, uint64_t* maskCopy, const void* weight, const void* bias, int C,
                                          int mult, int Hi, int Wi, const cbGeom* geom, int act, int dtype,
                                          cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && outputState && weight && bits && maskCopy && bits != maskCopy && capN >= 0);
    // (allPixels: the producer's changes are not read)
    CB_REQUIRE(allPixels || ((changeIndexes != nullptr) != (inputMask != nullptr) && (!inputMask || !countDev)));
    CB_REQUIRE(inputMask != bits && inputMask != maskCopy);
    int Ho, Wo;
    int st = cbdw_shape(C, mult, Hi, Wi, geom, act, dtype, &Ho, &Wo);
    if (st != CB_OK) return st;
    cbPool win;
    if (!cbdw_window(*geom, &win)) return CB_ERR_UNSUPPORTED;
    CB_REQUIRE((long)Hi * Wi < (1l << 31));
    if (allPixels)
        return cbdw_take_and_launch(input, weight, bias, outputState, bits, maskCopy, 1, C * mult, mult, Hi, Wi, Ho, Wo,
                                    *geom, act, dtype, (hipStream_t)stream);
    st = cbinfer_pool_footprint(changeIndexes, capN, countDev, inputMask, Hi, Wi, &win, bits, stream);
    if (st != CB_OK) return st;
    return cbinfer_dwconv_changed(input, weight, bias, outputState, nullptr, bits, maskCopy, C, mult, Hi, Wi, geom, act,
                                  dtype, stream);
}

}  // extern "C"
