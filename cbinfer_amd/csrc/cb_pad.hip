// Change-based padding on gfx950: F.pad of a [C, H, W] map by (left, right, top, bottom) in the modes
// constant (with a value; negative pads crop), reflect, replicate and circular -- nn.ReflectionPad2d, nn.ReplicationPad2d,
// nn.ZeroPad2d, nn.ConstantPad2d, nn.CircularPad2d and what torch runs for nn.Conv2d(padding_mode != 'zeros').  The
// reference has none of them; contracts of the entry points in include/cbinfer_hip.h.  A pad computes nothing, and every
// producer of this library leaves the pixels outside its change list bit for bit as they were, so the output can differ
// from last frame's only at the FOOTPRINT of the input's changes on the output map; copying there gives the dense result
// exactly, without a threshold.  A frame is
//   an input in LIST form, one launch in front: the list's footprint ORed into the zeroed working mask of the OUTPUT map
//              (one thread per entry; per axis an input coordinate is read by at most three intervals of output
//              coordinates -- its own image and up to two reflections / wraps, or the replicated border run contiguous
//              with the image --, one 64-bit atomicOr per mask word an interval touches);
//   one launch, mask-driven: the word walk of cb_maskwalk.h (cb_walk_words) over the OUTPUT mask words, the launch shape
//              of cb_rearrange.hip.  Lane j of every wave owns output column 64 tile + j, derives its source column -- the
//              source row is uniform for the word --, tests that bit of the input mask and one ballot makes the word; an
//              item is (set bit, four output channels): four loads, then four stores.
// No LDS, host sync, memset, allocation, data atomics or inline assembly.
#include "cb_maskwalk.h"

namespace {

#define CBP_MAXPAD 64     // |pad| limit: cbGeom's padding bound
#define CBP_GROUP 4       // output channels copied per item of the word walk

// The source coordinate of output coordinate o on an axis of n input pixels with the leading pad p, or -1 where the
// pixel reads no input (constant mode outside the image).  Within the limits of cbinfer_pad_supported the result lies in
// 0 .. n - 1: reflect has p and the trailing pad below n, so |o - p| <= 2 n - 2; circular has them <= n, so
// -n <= o - p <= 2 n - 1.
template <int MODE>
__device__ __forceinline__ int cbp_source(int o, int p, int n) {
    int i = o - p;
    if (MODE == CB_PAD_CONSTANT) return (unsigned)i < (unsigned)n ? i : -1;
    if (MODE == CB_PAD_REFLECT) {
        i = i < 0 ? -i : i;
        return i >= n ? 2 * (n - 1) - i : i;
    }
    if (MODE == CB_PAD_REPLICATE) return min(max(i, 0), n - 1);
    return i < 0 ? i + n : (i >= n ? i - n : i);
}

// The output coordinates that read input coordinate i of an axis (n input pixels, pads p in front and q behind) as three
// intervals lo[k] .. hi[k], cut to the output 0 .. n + p + q - 1; an empty one has lo > hi.
__device__ __forceinline__ void cbp_readers(int mode, int i, int n, int p, int q, int (&lo)[3], int (&hi)[3]) {
    const int N = n + p + q;
    lo[0] = hi[0] = i + p;      // its own image (constant: cropped away where a pad is negative)
    lo[1] = lo[2] = 0;
    hi[1] = hi[2] = -1;
    if (mode == CB_PAD_REFLECT) {
        if (i >= 1 && i <= p) lo[1] = hi[1] = p - i;                                       // o - p = -i
        if (i <= n - 2 && i >= n - 1 - q) lo[2] = hi[2] = 2 * (n - 1) - i + p;             // o - p = 2 (n - 1) - i
    } else if (mode == CB_PAD_REPLICATE) {
        if (i == 0) lo[0] = 0;              // the border run is contiguous with the image: up to 65 coordinates,
        if (i == n - 1) hi[0] = N - 1;      // 129 with n == 1
    } else if (mode == CB_PAD_CIRCULAR) {
        if (i >= n - p) lo[1] = hi[1] = i - n + p;                                         // o - p = i - n
        if (i < q) lo[2] = hi[2] = i + n + p;                                              // o - p = i + n
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = max(lo[k], 0);
        hi[k] = min(hi[k], N - 1);
    }
}

// List form: one thread per list entry ORs the entry's footprint into `bits`, the working mask of the Ho x Wo output
// map (wprO words per row).  Every row and column written lies inside the output map (cbp_readers cuts them).
__global__ __launch_bounds__(256) void cbp_footprint_kernel(const int32_t* __restrict__ list, int nHost,
                                                           const int32_t* __restrict__ countDev, int H, int W, int mode,
                                                           int left, int right, int top, int bottom, int wprO,
                                                           unsigned long long* __restrict__ bits) {
    const int N = countDev ? min(*countDev, nHost) : nHost;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (long)gridDim.x * blockDim.x) {
        const int pos = list[e];
        if ((unsigned)pos >= (unsigned)(H * W)) continue;      // (an out-of-map entry is dropped)
        const int y = pos / W, x = pos - y * W;
        int yLo[3], yHi[3], xLo[3], xHi[3];
        cbp_readers(mode, y, H, top, bottom, yLo, yHi);
        cbp_readers(mode, x, W, left, right, xLo, xHi);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            for (int oy = yLo[a]; oy <= yHi[a]; ++oy) {
                unsigned long long* row = bits + (long)oy * wprO;
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    for (int w = xLo[b] >> 6; xLo[b] <= xHi[b] && w <= xHi[b] >> 6; ++w) {      // (at most three words)
                        const int first = max(xLo[b] - w * 64, 0), last = min(xHi[b] - w * 64, 63);
                        atomicOr(row + w, (~0ull << first) & (~0ull >> (63 - last)));
                    }
            }
    }
}

// in [C, H, W], out [C, Ho, Wo]: out[c, oy, ox] = in[c, source(oy), source(ox)], or `value` where constant mode reads no
// input.  inMask: the input's change mask of this frame (row-padded over the INPUT map), or NULL; all: every output
// pixel is listed.  An input in list form has its footprint in `bits` already.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void cbp_pad_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                     const unsigned long long* __restrict__ inMask, int all,
                                                     unsigned long long* bits, unsigned long long* __restrict__ maskCopy,
                                                     long words, int C, int H, int W, int left, int top, float value,
                                                     int Ho, int Wo, int wprI, int wprO) {
    const long HWi = (long)H * W, HWo = (long)Ho * Wo;
    const int lane = threadIdx.x & 63;
    const T fill = (T)value;      // (converted once, round to nearest even)
    cb_walk_words(
        bits, maskCopy, words, (C + CBP_GROUP - 1) / CBP_GROUP, Wo, wprO, all,
        [&](long w, int oy, int tile) {
            if (!inMask) return 0ull;
            // every wave makes the same word: lane j tests the input change bit that output column 64 tile + j reads.
            // The source columns of a word may lie in another input word, in two, or run backwards: indexed per lane.
            const int sy = cbp_source<MODE>(oy, top, H);
            const int ox = tile * 64 + lane;
            const int sx = ox < Wo ? cbp_source<MODE>(ox, left, W) : -1;
            bool bit = false;
            if (sy >= 0 && sx >= 0) bit = (inMask[(long)sy * wprI + (sx >> 6)] >> (sx & 63) & 1ull) != 0;
            return (unsigned long long)__ballot(bit);
        },
        [&](int cg, int oy, int ox) {
            // CBP_GROUP channels per item, their loads requested before the first store (a channel beyond the end loads
            // the last channel again and stores nothing; a pixel that reads no input loads pixel 0 and stores `value`:
            // only an every-pixel frame lists such a pixel)
            const int sy = cbp_source<MODE>(oy, top, H), sx = cbp_source<MODE>(ox, left, W);
            const bool reads = sy >= 0 && sx >= 0;
            const long src = reads ? (long)sy * W + sx : 0;
            T v[CBP_GROUP];
#pragma unroll
            for (int u = 0; u < CBP_GROUP; ++u) v[u] = in[(long)min(cg * CBP_GROUP + u, C - 1) * HWi + src];
            const long dst = (long)oy * Wo + ox;
#pragma unroll
            for (int u = 0; u < CBP_GROUP; ++u)      // (a copy: bit for bit)
                if (cg * CBP_GROUP + u < C) out[(long)(cg * CBP_GROUP + u) * HWo + dst] = reads ? v[u] : fill;
        });
}

template <typename T>
void cbp_launch(const void* in, void* out, const uint64_t* inMask, int all, uint64_t* bits, uint64_t* maskCopy, int C,
                int H, int W, int Ho, int Wo, const cbPad& p, hipStream_t s) {
    const int wprO = (Wo + 63) / 64, wprI = (W + 63) / 64;
    const long words = (long)Ho * wprO;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBP_GO(MODE)                                                                                                  \
    hipLaunchKernelGGL((cbp_pad_kernel<T, MODE>), grid, block, 0, s, (const T*)in, (T*)out,                          \
                       (const unsigned long long*)inMask, all, (unsigned long long*)bits,                            \
                       (unsigned long long*)maskCopy, words, C, H, W, p.left, p.top, p.value, Ho, Wo, wprI, wprO)
    switch (p.mode) {
        case CB_PAD_CONSTANT: CBP_GO(CB_PAD_CONSTANT); break;
        case CB_PAD_REFLECT: CBP_GO(CB_PAD_REFLECT); break;
        case CB_PAD_REPLICATE: CBP_GO(CB_PAD_REPLICATE); break;
        default: CBP_GO(CB_PAD_CIRCULAR); break;
    }
#undef CBP_GO
}

}  // namespace

int cbinfer_pad_supported(const cbPad* p, int H, int W) {
    if (!p || H < 1 || W < 1) return 0;
    if (p->mode != CB_PAD_CONSTANT && p->mode != CB_PAD_REFLECT && p->mode != CB_PAD_REPLICATE &&
        p->mode != CB_PAD_CIRCULAR)
        return 0;
    const int pads[4] = {p->left, p->right, p->top, p->bottom}, extent[4] = {W, W, H, H};
    for (int k = 0; k < 4; ++k) {
        if (pads[k] < -CBP_MAXPAD || pads[k] > CBP_MAXPAD) return 0;
        if (p->mode != CB_PAD_CONSTANT && pads[k] < 0) return 0;      // (cropping: constant mode only)
        if (p->mode == CB_PAD_REFLECT && pads[k] >= extent[k]) return 0;
        if (p->mode == CB_PAD_CIRCULAR && pads[k] > extent[k]) return 0;
    }
    return (long)H + p->top + p->bottom >= 1 && (long)W + p->left + p->right >= 1 &&
           (long)H + p->top + p->bottom < (1l << 31) && (long)W + p->left + p->right < (1l << 31);
}

int cbinfer_pad_out_size(const cbPad* p, int H, int W, int* Ho, int* Wo) {
    CB_REQUIRE(p && Ho && Wo && H >= 1 && W >= 1);
    if (!cbinfer_pad_supported(p, H, W)) return CB_ERR_UNSUPPORTED;
    *Ho = H + p->top + p->bottom, *Wo = W + p->left + p->right;
    return CB_OK;
}

int cbinfer_cbpad_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list, int capN,
                          const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, const cbPad* p,
                          int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && outputState && input != outputState && bits && maskCopy && bits != maskCopy && C >= 1 && H >= 1 &&
               W >= 1);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_pad_supported(p, H, W));
    CB_REQUIRE(capN >= 0 && !(inputMask && list) && (list || !countDev));
    CB_REQUIRE(inputMask != bits && inputMask != maskCopy);
    const int Ho = H + p->top + p->bottom, Wo = W + p->left + p->right;
    // (a list addresses a pixel of the input map with an int32, the list made from maskCopy one of the output map; the
    //  kernel numbers a word's items with an int)
    CB_REQUIRE((long)Ho * Wo < (1l << 31) && (long)H * W < (1l << 31) && (long)C * 64 < (1l << 31));
    const int all = !inputMask && !list;
    if (list && capN > 0) {
        long blocks = ((long)capN + 255) / 256;
        if (blocks > 256 * 8) blocks = 256 * 8;
        hipLaunchKernelGGL(cbp_footprint_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, list, capN,
                           countDev, H, W, p->mode, p->left, p->right, p->top, p->bottom, (Wo + 63) / 64,
                           (unsigned long long*)bits);
        const int st = cb_launch_status();
        if (st != CB_OK) return st;
    }
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbp_launch<decltype(t)>(input, outputState, inputMask, all, bits, maskCopy, C, H, W, Ho, Wo, *p,
                                (hipStream_t)stream);
    });
    return cb_launch_status();
}
