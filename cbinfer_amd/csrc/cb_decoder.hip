// Change-based upsampling (nearest, bilinear; integer scales 1..8 per axis) and channel concatenation of 2..4 maps on
// gfx950: the two operators a decoder -- FCN / DeepLab head, U-Net, FPN top-down path -- adds to an
// encoder.  The reference has neither; contracts of the entry points in include/cbinfer_hip.h.  Every producer of this
// library leaves the pixels outside its change list bit for bit as they were, so the output of either operator can
// differ from last frame's only at the FOOTPRINT of the operands' changes: recomputing there gives the dense result
// exactly, without a threshold.  A frame is
//   per operand in LIST form, one launch in front: the list's footprint ORed into a zeroed working mask of the OUTPUT
//              map (upsample: the output pixels that read a listed input pixel, one thread per (entry, candidate output
//              row), at most two 64-bit atomicOr per row; concat: cb_list_to_bits of cb_maskwalk.h into the operand's
//              own working mask);
//   one launch, mask-driven: workgroups of four waves stride over the output mask words.  Upsample is the word walk of
//              cb_maskwalk.h (cb_walk_words): lane j of every wave owns output column 64 w + j of the word, tests the
//              input change bits of its source pixels, and one ballot makes the word (cbp2_footprint_mask_kernel's
//              scheme in front of the recompute).  Concat keeps a loop of its own in the walk's order: every operand
//              has a word of its own -- its channels are copied at ITS pixels only -- and the union is handed on; the
//              word's owner writes the frame's mask copy and zeroes the working words it used.
// No host sync, memset, allocation, data atomics or inline assembly.
#include "cb_maskwalk.h"

namespace {

#define CBU_MAXS 8      // scale limit per axis
#define CBC_MAXN 4      // operands of a concat

// ---------------------------------------------------------------------------------------------------- upsample
// MODE 0: nearest; 1: bilinear, align_corners=False; 2: bilinear, align_corners=True.
// The two source coordinates of output coordinate o on an axis of n input and N = n s output pixels, and the numerator
// rho and denominator den of the second one's weight -- all in integers (nearest: i1 = i0 = o / s).
template <int MODE>
__device__ __forceinline__ void cbu_source(int o, int n, int s, int N, int& i0, int& i1, int& rho, int& den) {
    if (MODE == 0) {
        i0 = i1 = o / s;
        rho = 0, den = 1;
        return;
    }
    long num;
    if (MODE == 1) {
        num = 2 * (long)o + 1 - s;
        num = num > 0 ? num : 0;
        den = 2 * s;
    } else {
        num = N > 1 ? (long)o * (n - 1) : 0l;
        den = N > 1 ? N - 1 : 1;
    }
    i0 = (int)(num / den);
    rho = (int)(num - (long)i0 * den);
    i1 = min(i0 + 1, n - 1);
}

// List form: one thread per (list entry, r-th candidate output row), r < R.  The output rows that read input row y lie
// in [y sH, y sH + sH) for nearest and inside [(y - 2) sH, (y + 4) sH] for bilinear (the source coordinate advances by
// 1 / s per output pixel with align_corners=False and by (n - 1) / (N - 1) in (1 / (2 s), 1 / s] with True, and
// y (N - 1) / (n - 1) < y s + s); every candidate is TESTED with cbu_source, the range only has to hold them all.  The
// columns likewise: at most 6 sW + 1 <= 49 consecutive candidates, at most two words.
template <int MODE>
__global__ __launch_bounds__(256) void cbu_footprint_list_kernel(const int32_t* __restrict__ list, int nHost,
                                                                const int32_t* __restrict__ countDev, int Hi, int Wi,
                                                                int sH, int sW, int Ho, int Wo, int wprO, int R,
                                                                unsigned long long* __restrict__ bits) {
    const int N = countDev ? min(*countDev, nHost) : nHost;
    const long total = (long)N * R;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / R), r = (int)(i - (long)n * R);
        const int pos = list[n];
        if ((unsigned)pos >= (unsigned)(Hi * Wi)) continue;      // (an out-of-map entry is dropped)
        const int y = pos / Wi, x = pos - y * Wi;
        const int oy = (MODE == 0 ? y * sH : (y - 2) * sH) + r;
        if (oy < 0 || oy >= Ho) continue;
        int i0, i1, rho, den;
        cbu_source<MODE>(oy, Hi, sH, Ho, i0, i1, rho, den);
        if (i0 != y && i1 != y) continue;
        const int oxLo = max(MODE == 0 ? x * sW : (x - 2) * sW, 0);
        const int oxHi = min(MODE == 0 ? x * sW + sW - 1 : (x + 4) * sW, Wo - 1);
        const int w0 = oxLo >> 6;
        unsigned long long m0 = 0ull, m1 = 0ull;
        for (int ox = oxLo; ox <= oxHi; ++ox) {
            cbu_source<MODE>(ox, Wi, sW, Wo, i0, i1, rho, den);
            if (i0 == x || i1 == x) {
                if ((ox >> 6) == w0)
                    m0 |= 1ull << (ox & 63);
                else
                    m1 |= 1ull << (ox & 63);
            }
        }
        if (m0) atomicOr(bits + (long)oy * wprO + w0, m0);
        if (m1) atomicOr(bits + (long)oy * wprO + w0 + 1, m1);
    }
}

// in [C, Hi, Wi], out [C, Ho, Wo].  inMask: the input's change mask of this frame (row-padded over the INPUT map), or
// NULL; all: the input lists every pixel.  An input in list form has its footprint in `bits` already.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void cbu_upsample_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                          const unsigned long long* __restrict__ inMask, int all,
                                                          unsigned long long* bits,
                                                          unsigned long long* __restrict__ maskCopy, long words, int C,
                                                          int Hi, int Wi, int sH, int sW, int Ho, int Wo, int wprI,
                                                          int wprO) {
    const long HWi = (long)Hi * Wi, HWo = (long)Ho * Wo;
    const int lane = threadIdx.x & 63;
    int y0, y1, rhoY, denY;      // the source rows of the word's output row: made by makeWord, read by the items
    cb_walk_words(
        bits, maskCopy, words, C, Wo, wprO, all,
        [&](long, int oy, int tile) {
            cbu_source<MODE>(oy, Hi, sH, Ho, y0, y1, rhoY, denY);
            if (!inMask) return 0ull;
            // every wave makes the same word: lane j tests the change bits of the source pixels of column 64 tile + j
            const int ox = tile * 64 + lane;
            bool bit = false;
            if (ox < Wo) {
                int x0, x1, rho, den;
                cbu_source<MODE>(ox, Wi, sW, Wo, x0, x1, rho, den);
                const unsigned long long* r0 = inMask + (long)y0 * wprI;
                const unsigned long long* r1 = inMask + (long)y1 * wprI;
                const unsigned long long m = (r0[x0 >> 6] | r1[x0 >> 6]) >> (x0 & 63) |
                                             (r0[x1 >> 6] | r1[x1 >> 6]) >> (x1 & 63);
                bit = (m & 1ull) != 0;
            }
            return (unsigned long long)__ballot(bit);
        },
        [&](int c, int oy, int ox) {
            int x0, x1, rho, den;
            cbu_source<MODE>(ox, Wi, sW, Wo, x0, x1, rho, den);
            const T* src = in + (long)c * HWi;
            T res;
            if (MODE == 0) {
                res = src[(long)y0 * Wi + x0];      // (a copy: bit for bit)
            } else {
                // lambda = rho / den, one IEEE division; the value in f32, rounded to T once
                const float ly = __fdiv_rn((float)rhoY, (float)denY), lx = __fdiv_rn((float)rho, (float)den);
                const float a = cb_load_f32(src + (long)y0 * Wi + x0), b = cb_load_f32(src + (long)y0 * Wi + x1);
                const float cc = cb_load_f32(src + (long)y1 * Wi + x0), d = cb_load_f32(src + (long)y1 * Wi + x1);
                const float top = (1.f - lx) * a + lx * b, bot = (1.f - lx) * cc + lx * d;
                res = (T)((1.f - ly) * top + ly * bot);
            }
            out[(long)c * HWo + (long)oy * Wo + ox] = res;
        });
}

inline int cbu_mode(const cbUpsample& u) {
    return u.mode == CB_UPSAMPLE_NEAREST ? 0 : (u.alignCorners ? 2 : 1);
}

template <typename T>
void cbu_launch(const void* in, void* out, const uint64_t* inMask, int all, uint64_t* bits, uint64_t* maskCopy, int C,
                int Hi, int Wi, const cbUpsample& u, hipStream_t s) {
    const int Ho = Hi * u.sH, Wo = Wi * u.sW;
    const int wprO = (Wo + 63) / 64, wprI = (Wi + 63) / 64;
    const long words = (long)Ho * wprO;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBU_GO(MODE)                                                                                                  \
    hipLaunchKernelGGL((cbu_upsample_kernel<T, MODE>), grid, block, 0, s, (const T*)in, (T*)out,                     \
                       (const unsigned long long*)inMask, all, (unsigned long long*)bits,                            \
                       (unsigned long long*)maskCopy, words, C, Hi, Wi, u.sH, u.sW, Ho, Wo, wprI, wprO)
    switch (cbu_mode(u)) {
        case 0: CBU_GO(0); break;
        case 1: CBU_GO(1); break;
        default: CBU_GO(2); break;
    }
#undef CBU_GO
}

void cbu_launch_list(const int32_t* list, int cap, const int32_t* count, uint64_t* bits, int Hi, int Wi,
                     const cbUpsample& u, hipStream_t s) {
    const int Ho = Hi * u.sH, Wo = Wi * u.sW, wprO = (Wo + 63) / 64;
    const int mode = cbu_mode(u);
    const int R = mode == 0 ? u.sH : 6 * u.sH + 1;
    long blocks = ((long)cap * R + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    const dim3 grid((unsigned)blocks), block(256);
#define CBU_GO(MODE)                                                                                                  \
    hipLaunchKernelGGL((cbu_footprint_list_kernel<MODE>), grid, block, 0, s, list, cap, count, Hi, Wi, u.sH, u.sW, Ho, \
                       Wo, wprO, R, (unsigned long long*)bits)
    switch (mode) {
        case 0: CBU_GO(0); break;
        case 1: CBU_GO(1); break;
        default: CBU_GO(2); break;
    }
#undef CBU_GO
}

// ---------------------------------------------------------------------------------------------------- concat
struct cbc_operands {
    const void* src[CBC_MAXN];
    const unsigned long long* mask[CBC_MAXN];      // the operand's change mask of this frame, or NULL
    int channels[CBC_MAXN], first[CBC_MAXN];       // its channel count, its first channel in `out`
    int all[CBC_MAXN];                             // the operand lists every pixel
    int n;
};

// out [sum Ck, H, W].  bits: n working masks of `words` words, operand k's at bits + k words -- an operand in list form
// has its bits there already.
template <typename T>
__global__ __launch_bounds__(256) void cbc_concat_kernel(cbc_operands ops, T* __restrict__ out, unsigned long long* bits,
                                                        unsigned long long* __restrict__ maskCopy, long words, int H,
                                                        int W, int wpr) {
    const long HW = (long)H * W;
    for (long w = blockIdx.x; w < words; w += gridDim.x) {
        const int y = (int)(w / wpr), tile = (int)(w - (long)y * wpr);
        const unsigned long long valid = cb_valid_mask(W, tile);
        const long rowBase = (long)y * W + tile * 64;
        unsigned long long ownAny = 0ull, uni = 0ull;
#pragma unroll
        for (int k = 0; k < CBC_MAXN; ++k) {
            if (k >= ops.n) break;
            // (uniform over the workgroup: the working words are zeroed only behind the barrier below)
            const unsigned long long own = bits[k * words + w];
            unsigned long long word = own;
            if (ops.mask[k]) word |= ops.mask[k][w];
            word = ops.all[k] ? valid : (word & valid);      // (the bits of the row padding are never set)
            ownAny |= own;
            uni |= word;
            if (word != 0) {
                // operand k's channels at operand k's pixels: a copy, bit for bit
                const T* src = (const T*)ops.src[k];
                T* dst = out + (long)ops.first[k] * HW;
                const int n = __popcll(word);
                const int total = n * ops.channels[k];
                // four items per thread and round, the four loads requested before the first store: a copy is nothing
                // but memory round trips (an item beyond the end loads the thread's first item again and stores nothing)
                for (int e0 = threadIdx.x; e0 < total; e0 += 4 * 256) {
                    long o[4];
                    T v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int e = e0 + 256 * j < total ? e0 + 256 * j : e0;
                        const int c = e / n, i = e - c * n;
                        o[j] = (long)c * HW + rowBase + (n == 64 ? i : cb_select_bit(word, i));
                        v[j] = src[o[j]];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (e0 + 256 * j < total) dst[o[j]] = v[j];
                }
            }
        }
        if (threadIdx.x == 0) maskCopy[w] = uni;
        if (ownAny != 0) {
            __syncthreads();      // every wave has read the words
            if ((int)threadIdx.x < ops.n) bits[threadIdx.x * words + w] = 0;
        }
    }
}

template <typename T>
void cbc_launch(const cbc_operands& ops, void* out, uint64_t* bits, uint64_t* maskCopy, int H, int W, hipStream_t s) {
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    hipLaunchKernelGGL((cbc_concat_kernel<T>), dim3(cb_walk_grid(words)), dim3(256), 0, s, ops, (T*)out,
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, H, W, wpr);
}

}  // namespace

int cbinfer_upsample_supported(const cbUpsample* up) {
    if (!up) return 0;
    return up->sH >= 1 && up->sH <= CBU_MAXS && up->sW >= 1 && up->sW <= CBU_MAXS &&
           (up->mode == CB_UPSAMPLE_NEAREST || up->mode == CB_UPSAMPLE_BILINEAR) &&
           (up->alignCorners == 0 || up->alignCorners == 1);
}

int cbinfer_cbupsample_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list,
                               int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int Hi,
                               int Wi, const cbUpsample* up, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && outputState && bits && maskCopy && bits != maskCopy && C >= 1 && Hi >= 1 && Wi >= 1);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_upsample_supported(up));
    CB_REQUIRE(capN >= 0 && !(inputMask && list) && (list || !countDev));
    CB_REQUIRE(inputMask != bits && inputMask != maskCopy);
    // (a list addresses a pixel with an int32; the kernel numbers a word's items with an int)
    CB_REQUIRE((long)Hi * up->sH * ((long)Wi * up->sW) < (1l << 31) && (long)C * 64 < (1l << 31));
    const int all = !inputMask && !list;
    if (list && capN > 0) {
        cbu_launch_list(list, capN, countDev, bits, Hi, Wi, *up, (hipStream_t)stream);
        const int st = cb_launch_status();
        if (st != CB_OK) return st;
    }
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbu_launch<decltype(t)>(input, outputState, inputMask, all, bits, maskCopy, C, Hi, Wi, *up, (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbconcat_forward(const void* const* sources, const int32_t* channels, int n, void* outputState,
                             const uint64_t* const* masks, const int32_t* const* lists, const int32_t* caps,
                             const int32_t* const* counts, uint64_t* bits, uint64_t* maskCopy, int H, int W, int dtype,
                             cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(sources && channels && outputState && bits && maskCopy && n >= 2 && n <= CBC_MAXN && H >= 1 && W >= 1);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE((long)H * W < (1l << 31));
    const long words = (long)H * ((W + 63) / 64);
    CB_REQUIRE(maskCopy < bits || maskCopy >= bits + n * words);
    cbc_operands ops = {};
    ops.n = n;
    long total = 0;
    for (int k = 0; k < n; ++k) {
        const uint64_t* mask = masks ? masks[k] : nullptr;
        const int32_t* list = lists ? lists[k] : nullptr;
        const int32_t* count = counts ? counts[k] : nullptr;
        CB_REQUIRE(sources[k] && channels[k] >= 1 && (!caps || caps[k] >= 0));
        CB_REQUIRE(!(mask && list) && (list || !count));
        CB_REQUIRE(!mask || (mask != maskCopy && (mask < bits || mask >= bits + n * words)));
        ops.src[k] = sources[k];
        ops.mask[k] = (const unsigned long long*)mask;
        ops.channels[k] = channels[k];
        ops.first[k] = (int)total;
        ops.all[k] = !mask && !list;
        total += channels[k];
        CB_REQUIRE(total * 64 < (1l << 31));      // (the kernel numbers a word's items with an int)
    }
    for (int k = 0; k < n; ++k)
        if (lists && lists[k]) {
            const int st = cb_list_to_bits(lists[k], caps ? caps[k] : 0, counts ? counts[k] : nullptr, H, W,
                                           bits + k * words, stream);
            if (st != CB_OK) return st;
        }
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbc_launch<decltype(t)>(ops, outputState, bits, maskCopy, H, W, (hipStream_t)stream);
    });
    return cb_launch_status();
}
