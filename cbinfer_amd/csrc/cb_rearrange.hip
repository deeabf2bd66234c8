// Change-based pixel shuffle, pixel unshuffle and channel shuffle on gfx950: the three pure rearrangements
// of values -- nn.PixelShuffle (the upsampler of ESPCN / EDSR-type networks), nn.PixelUnshuffle (space-to-depth) and
// nn.ChannelShuffle (the middle of a ShuffleNet unit).  The reference has none of them; contracts of the entry points in
// include/cbinfer_hip.h.  Every producer of this library leaves the pixels outside its change list bit for bit as they
// were, so the output of a rearrangement can differ from last frame's only at the FOOTPRINT of the input's changes on
// the output map; copying there gives the dense result exactly, without a threshold.  A frame is
//   an input in LIST form, one launch in front: the list's footprint ORed into the zeroed working mask of the OUTPUT map
//              (shuffle: the r x r block of every entry, one thread per (entry, row of the block), at most two 64-bit
//              atomicOr per row; unshuffle: the footprint of an r x r / stride-r window, cbinfer_pool_footprint; channel
//              shuffle: the pixel itself, cb_list_to_bits);
//   one launch, mask-driven: the word walk of cb_maskwalk.h (cb_walk_words) over the OUTPUT mask words, the launch shape
//              of cb_decoder.hip's nearest upsampling.  Lane j of every wave owns output column 64 tile + j, tests the
//              input change bits that column reads and one ballot makes the word; an item is (set bit, four output
//              channels): four loads, then four stores.
// No LDS, host sync, memset, allocation, data atomics or inline assembly.
#include "cb_maskwalk.h"

namespace {

#define CBR_MAXF 8      // factor limit of the two pixel shuffles (CBUpsample2d's scale limit)
#define CBR_GROUP 4     // output channels copied per item of the word walk

// List form of the shuffle: one thread per (list entry, i-th row of its r x r output block), i < r.  The block's columns
// are r <= 8 consecutive bits: at most two words (r = 3, 5, 6, 7 can straddle).
__global__ __launch_bounds__(256) void cbr_shuffle_footprint_kernel(const int32_t* __restrict__ list, int nHost,
                                                                   const int32_t* __restrict__ countDev, int Hi, int Wi,
                                                                   int r, int wprO, unsigned long long* __restrict__ bits) {
    const int N = countDev ? min(*countDev, nHost) : nHost;
    const long total = (long)N * r;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int n = (int)(e / r), i = (int)(e - (long)n * r);
        const int pos = list[n];
        if ((unsigned)pos >= (unsigned)(Hi * Wi)) continue;      // (an out-of-map entry is dropped)
        const int y = pos / Wi, x = pos - y * Wi;
        const int oy = y * r + i, oxLo = x * r, oxHi = x * r + r - 1;      // (inside the output map: Ho = Hi r, Wo = Wi r)
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

// KIND (CB_REARRANGE_*) with factor f; in [Ci, Hi, Wi], out [Co, Ho, Wo]:
//   SHUFFLE    Ci = Co f f, Ho = Hi f, Wo = Wi f:  out[c, y f + i, x f + j] = in[c f f + i f + j, y, x]
//   UNSHUFFLE  Co = Ci f f, Hi = Ho f, Wi = Wo f:  out[c f f + i f + j, y, x] = in[c, y f + i, x f + j]
//   CHANNELS   the same shape, n = Co / f:         out[k f + q] = in[q n + k], q < f, k < n
// inMask: the input's change mask of this frame (row-padded over the INPUT map), or NULL; all: the input lists every
// pixel.  An input in list form has its footprint in `bits` already.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void cbr_rearrange_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                           const unsigned long long* __restrict__ inMask, int all,
                                                           unsigned long long* bits,
                                                           unsigned long long* __restrict__ maskCopy, long words, int Co,
                                                           int Hi, int Wi, int f, int Ho, int Wo, int wprI, int wprO) {
    const long HWi = (long)Hi * Wi, HWo = (long)Ho * Wo;
    const int lane = threadIdx.x & 63;
    const int ff = f * f, perGroup = Co / f;
    cb_walk_words(
        bits, maskCopy, words, (Co + CBR_GROUP - 1) / CBR_GROUP, Wo, wprO, all,
        [&](long w, int oy, int tile) {
            if (!inMask) return 0ull;
            if (KIND == CB_REARRANGE_CHANNELS) return inMask[w];      // (the same map: the input's word itself)
            // every wave makes the same word: lane j tests the input change bits that output column 64 tile + j reads
            const int ox = tile * 64 + lane;
            bool bit = false;
            if (ox < Wo) {
                if (KIND == CB_REARRANGE_SHUFFLE) {
                    const int x = ox / f;
                    bit = (inMask[(long)(oy / f) * wprI + (x >> 6)] >> (x & 63) & 1ull) != 0;
                } else {
                    // the f input rows of the block ORed, then the f bits from input column ox f on: they lie in one
                    // word, or (f = 3, 5, 6, 7) in two -- sh + f > 64 leaves 64 - sh in 1..7, never a shift by 64
                    const int x0 = ox * f, w0 = x0 >> 6, sh = x0 & 63;
                    const bool two = sh + f > 64 && w0 + 1 < wprI;
                    const unsigned long long* row = inMask + (long)oy * f * wprI + w0;
                    unsigned long long m0 = 0ull, m1 = 0ull;
                    for (int i = 0; i < f; ++i, row += wprI) {
                        m0 |= row[0];
                        if (two) m1 |= row[1];
                    }
                    unsigned long long v = m0 >> sh;
                    if (two) v |= m1 << (64 - sh);
                    bit = (v & ((1ull << f) - 1ull)) != 0;
                }
            }
            return (unsigned long long)__ballot(bit);
        },
        [&](int cg, int oy, int ox) {
            // CBR_GROUP channels per item, their loads requested before the first store: a copy is nothing but memory
            // round trips (a channel beyond the end loads the last channel again and stores nothing)
            T v[CBR_GROUP];
#pragma unroll
            for (int u = 0; u < CBR_GROUP; ++u) {
                const int c = min(cg * CBR_GROUP + u, Co - 1);
                long src;
                if (KIND == CB_REARRANGE_SHUFFLE) {
                    const int y = oy / f, i = oy - y * f, x = ox / f, j = ox - x * f;
                    src = ((long)c * ff + i * f + j) * HWi + (long)y * Wi + x;
                } else if (KIND == CB_REARRANGE_UNSHUFFLE) {
                    const int ci = c / ff, rem = c - ci * ff, i = rem / f, j = rem - i * f;
                    src = (long)ci * HWi + ((long)oy * f + i) * Wi + (long)ox * f + j;
                } else {
                    const int k = c / f, q = c - k * f;
                    src = ((long)q * perGroup + k) * HWi + (long)oy * Wi + ox;
                }
                v[u] = in[src];
            }
            const long dst = (long)oy * Wo + ox;
#pragma unroll
            for (int u = 0; u < CBR_GROUP; ++u)      // (a copy: bit for bit)
                if (cg * CBR_GROUP + u < Co) out[(long)(cg * CBR_GROUP + u) * HWo + dst] = v[u];
        });
}

template <typename T>
void cbr_launch(const void* in, void* out, const uint64_t* inMask, int all, uint64_t* bits, uint64_t* maskCopy, int Co,
                int Hi, int Wi, int Ho, int Wo, const cbRearrange& r, hipStream_t s) {
    const int wprO = (Wo + 63) / 64, wprI = (Wi + 63) / 64;
    const long words = (long)Ho * wprO;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBR_GO(KIND)                                                                                                  \
    hipLaunchKernelGGL((cbr_rearrange_kernel<T, KIND>), grid, block, 0, s, (const T*)in, (T*)out,                    \
                       (const unsigned long long*)inMask, all, (unsigned long long*)bits,                            \
                       (unsigned long long*)maskCopy, words, Co, Hi, Wi, r.factor, Ho, Wo, wprI, wprO)
    switch (r.kind) {
        case CB_REARRANGE_SHUFFLE: CBR_GO(CB_REARRANGE_SHUFFLE); break;
        case CB_REARRANGE_UNSHUFFLE: CBR_GO(CB_REARRANGE_UNSHUFFLE); break;
        default: CBR_GO(CB_REARRANGE_CHANNELS); break;
    }
#undef CBR_GO
}

// the list's footprint ORed into `bits`, the working mask of the output map (cap > 0)
int cbr_launch_list(const int32_t* list, int cap, const int32_t* count, uint64_t* bits, int Hi, int Wi, int Wo,
                    const cbRearrange& r, cbStream_t stream) {
    if (r.kind == CB_REARRANGE_CHANNELS) return cb_list_to_bits(list, cap, count, Hi, Wi, bits, stream);
    if (r.kind == CB_REARRANGE_UNSHUFFLE) {
        const cbPool window = {r.factor, r.factor, r.factor, r.factor, 0, 0, 0, CB_POOL_MAX};
        return cbinfer_pool_footprint(list, cap, count, nullptr, Hi, Wi, &window, bits, stream);
    }
    long blocks = ((long)cap * r.factor + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(cbr_shuffle_footprint_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, list, cap,
                       count, Hi, Wi, r.factor, (Wo + 63) / 64, (unsigned long long*)bits);
    return cb_launch_status();
}

}  // namespace

int cbinfer_rearrange_supported(const cbRearrange* r) {
    if (!r) return 0;
    if (r->kind == CB_REARRANGE_SHUFFLE || r->kind == CB_REARRANGE_UNSHUFFLE) return r->factor >= 1 && r->factor <= CBR_MAXF;
    return r->kind == CB_REARRANGE_CHANNELS && r->factor >= 1;
}

int cbinfer_rearrange_out_shape(const cbRearrange* r, int C, int H, int W, int* Co, int* Ho, int* Wo) {
    CB_REQUIRE(r && Co && Ho && Wo && C >= 1 && H >= 1 && W >= 1);
    if (!cbinfer_rearrange_supported(r)) return CB_ERR_UNSUPPORTED;
    const int f = r->factor;
    if (r->kind == CB_REARRANGE_SHUFFLE) {
        CB_REQUIRE(C % (f * f) == 0 && (long)H * f < (1l << 31) && (long)W * f < (1l << 31));
        *Co = C / (f * f), *Ho = H * f, *Wo = W * f;
    } else if (r->kind == CB_REARRANGE_UNSHUFFLE) {
        CB_REQUIRE(H % f == 0 && W % f == 0 && (long)C * f * f < (1l << 31));
        *Co = C * f * f, *Ho = H / f, *Wo = W / f;
    } else {
        CB_REQUIRE(C % f == 0);      // (and so f <= C)
        *Co = C, *Ho = H, *Wo = W;
    }
    return CB_OK;
}

int cbinfer_cbrearrange_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list,
                                int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W,
                                const cbRearrange* r, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && outputState && input != outputState && bits && maskCopy && bits != maskCopy && C >= 1 && H >= 1 &&
               W >= 1);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_rearrange_supported(r));
    CB_REQUIRE(capN >= 0 && !(inputMask && list) && (list || !countDev));
    CB_REQUIRE(inputMask != bits && inputMask != maskCopy);
    int Co, Ho, Wo;
    CB_REQUIRE(cbinfer_rearrange_out_shape(r, C, H, W, &Co, &Ho, &Wo) == CB_OK);
    // (a list addresses a pixel of the input map with an int32, the list made from maskCopy one of the output map; the
    //  kernel numbers a word's items with an int)
    CB_REQUIRE((long)Ho * Wo < (1l << 31) && (long)H * W < (1l << 31) && (long)Co * 64 < (1l << 31));
    const int all = !inputMask && !list;
    if (list && capN > 0) {
        const int st = cbr_launch_list(list, capN, countDev, bits, H, W, Wo, *r, stream);
        if (st != CB_OK) return st;
    }
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbr_launch<decltype(t)>(input, outputState, inputMask, all, bits, maskCopy, Co, H, W, Ho, Wo, *r,
                                (hipStream_t)stream);
    });
    return cb_launch_status();
}
