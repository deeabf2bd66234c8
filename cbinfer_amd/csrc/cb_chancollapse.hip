// Change-based reductions that COLLAPSE the channel axis of one pixel -- sum, mean, L2 norm, max, min over the channels
// (1 .. 4 of them from one pass, one output channel each) and argmax / argmin (an int64 label map) -- on gfx950
// (DESIGN 5.27).  The reference ends a frame with torch.max(y.cpu(), 1); contracts of the entry points in
// include/cbinfer_hip.h.  As for cb_chanreduce.hip the output at a pixel depends on the C values at that pixel alone, and
// every producer of this library leaves the pixels outside its change list bit for bit as they were: recomputing at the
// operand's changed pixels gives the dense result exactly, without a threshold.  A frame is
//   for an operand in LIST form, one launch in front: the list's bits ORed into the zeroed working mask
//              (cb_list_to_bits of cb_maskwalk.h);
//   one launch, the word-level walk of cb_maskwalk.h (cb_walk_word_units): the unit of work is a non-empty mask word,
//              up to 64 pixels of a row, lane <-> pixel.
// ONE pass over the C values: a thread folds the channels of its slices (c mod 16, ascending c) into a sum and a sum of
// squares, into the two (value, index) extremes, or into both groups, the partials meet in LDS behind one barrier, and
// the pixel's first thread group finishes and stores.  The summation order is sum16 of DESIGN 5.21 and does not depend
// on the launch: a word with more than 16 listed pixels gives a thread four slices of one pixel, a word with at most 16
// gives it one, and both evaluate the same tree.  The extremes are combined under a total order on (value, index), which
// is associative: their result does not depend on the tree at all.  No held values, no dynamic LDS, no data atomics,
// host sync, memset, allocation or inline assembly; all stores are plain vector stores.
#include "cb_maskwalk.h"

// (everything is evaluated as written, one rounding per operation: cb_chanreduce.hip, cb_pointwise.hip)
#pragma clang fp contract(off)

namespace {

// What a call's kinds need of the pass decides the kernel: CBC_ARG, one extreme and its index (argmax / argmin); else
// CBC_SUMS, the sum and the sum of squares (sum, mean, norm), CBC_EXTREMES, both extremes (max, min), or both groups.
// Within a group everything is folded whether asked for or not: the pass is bound by its loads, and so its loop has no
// branch on the kinds.
enum { CBC_ARG = 0, CBC_SUMS = 1, CBC_EXTREMES = 2, CBC_BOTH = 3 };
inline int cbc_kind(int ops, int k) { return (ops >> (4 * k)) & 15; }
inline int cbc_mode(int ops, int nOps) {
    int mode = 0;
    for (int k = 0; k < nOps; ++k) {
        const int kind = cbc_kind(ops, k);
        mode |= kind <= CB_CC_NORM ? CBC_SUMS : kind <= CB_CC_MIN ? CBC_EXTREMES : CBC_ARG;
    }
    return mode;
}

// An extreme of the channels seen so far and where it stands.  torch's CPU order: a NaN beats every number, otherwise
// the larger (min: the smaller) value does; among equals -- two NaNs, or a == b, which +0 and -0 are -- the smaller
// index.  This is a total preorder on (value, index) whose ties the index breaks, so taking the better of two is
// associative and commutative: any tree over the channels gives the same pair.
// The order is held as ONE unsigned 64-bit key, larger is better (one comparison per channel; comparing value and index
// separately takes six lane masks, a scalar register pair each): in the high half the value's rank -- its bits (negated for a
// minimum, -0 taken as +0) mapped monotonically to an unsigned, every NaN to the top --, in the low half 2^31 - 1 - c,
// so that among equal ranks the smaller index wins.  Keys of different channels differ; the start key 0 is below the
// key of every channel (-inf ranks 0x007fffff).  The value itself travels beside the key: a rank does not tell -0.
struct cbc_best {
    unsigned long long key;
    float v;
};
__device__ __forceinline__ cbc_best cbc_start() { return {0ull, 0.f}; }
__device__ __forceinline__ cbc_best cbc_channel(float v, int c, bool isMin) {
    unsigned b = __float_as_uint(v) ^ (isMin ? 0x80000000u : 0u);
    const unsigned mag = b & 0x7fffffffu;
    b = mag == 0u ? 0u : b;                                               // -0 -> +0
    const unsigned ordered = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);      // monotone in the number
    const unsigned rank = mag > 0x7f800000u ? 0xffffffffu : ordered;     // a NaN beats every number
    return {((unsigned long long)rank << 32) | (unsigned)(0x7fffffff - c), v};
}
__device__ __forceinline__ cbc_best cbc_better(cbc_best a, cbc_best b) { return b.key > a.key ? b : a; }
__device__ __forceinline__ int cbc_index(cbc_best a) { return 0x7fffffff - (int)(unsigned)a.key; }

// p[2i] + p[2i+1], level by level, of N = 1, 4 or 16 neighbouring nodes of sum16's tree
template <int N>
__device__ __forceinline__ float cbc_tree(float (&p)[N]) {
#pragma unroll
    for (int m = N; m > 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < m / 2; ++i) p[i] = p[2 * i] + p[2 * i + 1];
    return p[0];
}

// The rows of a partials region, 256 words each, [thread group][pixel]: an extreme has three (the key's halves and the
// value; CBC_ARG needs no value: two), CBC_SUMS the two sums, CBC_EXTREMES two extremes, CBC_BOTH all eight.
template <int MODE>
struct cbc_rows {
    static constexpr int HI = 0, LO = 3, SUM = MODE == CBC_BOTH ? 6 : 0, SQ = SUM + 1;
    static constexpr int N = MODE == CBC_BOTH ? 8 : MODE == CBC_EXTREMES ? 6 : 2;
};

template <bool VALUE>
__device__ __forceinline__ void cbc_write(unsigned (*red)[256], int row, int slot, cbc_best a) {
    red[row][slot] = (unsigned)a.key;
    red[row + 1][slot] = (unsigned)(a.key >> 32);
    if (VALUE) red[row + 2][slot] = __float_as_uint(a.v);
}
template <bool VALUE>
__device__ __forceinline__ cbc_best cbc_read(unsigned (*red)[256], int row, int slot) {
    return {((unsigned long long)red[row + 1][slot] << 32) | red[row][slot],
            VALUE ? __uint_as_float(red[row + 2][slot]) : 0.f};
}

// One non-empty word.  SL = 4: 64 pixels, wave k owns the slices 4k .. 4k + 3;  SL = 1: 16 pixels, one slice per
// thread.  `red` is this word's partials region: the launch uses two in turn, so a region's partials are read behind ONE
// barrier and it is written again only behind the barrier of the word after it.
template <typename T, int MODE, int SL>
__device__ __forceinline__ void cbc_word(const T* __restrict__ x, void* __restrict__ out,
                                         unsigned long long* __restrict__ labelMask, long w, int all,
                                         unsigned long long word, int n, long first, long HW, int C, int ops, int nOps,
                                         unsigned (*red)[256]) {
    constexpr int PX = SL == 4 ? 64 : 16, NP = 16 / SL;
    constexpr bool ARG = MODE == CBC_ARG, SUMS = (MODE & CBC_SUMS) != 0, EXT = (MODE & CBC_EXTREMES) != 0;
    using rows = cbc_rows<MODE>;
    // (a wave of the four-slice form is one thread group: its channel numbers and their bounds are scalars)
    const int px = threadIdx.x & (PX - 1);
    const int grp = SL == 4 ? __builtin_amdgcn_readfirstlane(threadIdx.x / PX) : threadIdx.x / PX;
    const bool live = px < n;
    const int bit = n == 64 ? px : cb_select_bit(word, live ? px : 0);
    const T* xp = x + first + bit;
    // (an arg launch keeps its one extreme in `hi`, whichever it is)
    const bool hiMin = ARG && (ops & 15) == CB_CC_ARGMIN;
    float s[SL], q[SL];
    cbc_best hi[SL], lo[SL];
#pragma unroll
    for (int j = 0; j < SL; ++j) {
        s[j] = q[j] = 0.f;
        hi[j] = lo[j] = cbc_start();
    }
    // The thread's channels in batches of four loads that are requested together: the four slices of one round (SL = 4),
    // or four rounds of its one slice (SL = 1).  Either way a slice is folded in ascending c.
    const auto chan = [](int c0, int u) { return SL == 4 ? c0 + u : c0 + 16 * u; };
    const auto fold = [&](int u, int c, float v) {
        const int j = SL == 4 ? u : 0;
        if (SUMS) {
            const float vv = v * v;
            s[j] = s[j] + v;
            q[j] = q[j] + vv;
        }
        if (ARG || EXT) hi[j] = cbc_better(hi[j], cbc_channel(v, c, hiMin));
        if (EXT) lo[j] = cbc_better(lo[j], cbc_channel(v, c, true));
    };
    if (live) {
        int c0 = grp * SL;
        for (; chan(c0, 3) < C; c0 += SL == 4 ? 16 : 64) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = cb_load_f32(xp + (long)chan(c0, u) * HW);
#pragma unroll
            for (int u = 0; u < 4; ++u) fold(u, chan(c0, u), v[u]);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)      // (the last, partial batch: its fourth channel is beyond C)
            if (chan(c0, u) < C) fold(u, chan(c0, u), cb_load_f32(xp + (long)chan(c0, u) * HW));
    }
    // (the thread's slices are neighbouring nodes of the tree)
    const int slot = grp * PX + px;
    if (SUMS) {
        red[rows::SUM][slot] = __float_as_uint(cbc_tree<SL>(s));
        red[rows::SQ][slot] = __float_as_uint(cbc_tree<SL>(q));
    }
    if (ARG || EXT) {
#pragma unroll
        for (int j = 1; j < SL; ++j) hi[0] = cbc_better(hi[0], hi[j]);
        cbc_write<EXT>(red, rows::HI, slot, hi[0]);
    }
    if (EXT) {
#pragma unroll
        for (int j = 1; j < SL; ++j) lo[0] = cbc_better(lo[0], lo[j]);
        cbc_write<true>(red, rows::LO, slot, lo[0]);
    }
    __syncthreads();
    const bool writer = grp == 0 && live;      // the pixel's first thread group: along the word, contiguous stores
    cbc_best H = cbc_start(), L = cbc_start();
    if ((ARG || EXT) && writer)
#pragma unroll
        for (int i = 0; i < NP; ++i) H = cbc_better(H, cbc_read<EXT>(red, rows::HI, i * PX + px));
    if (ARG) {
        if (threadIdx.x >= 64) return;         // (both forms have their writers in wave 0)
        unsigned long long moved = 0ull;
        if (writer) {
            long long* op = (long long*)out + first + bit;
            // (the label the state held before the launch: read by the thread that writes it)
            const long long label = cbc_index(H);
            if (labelMask && (all || *op != label)) moved = 1ull << bit;
            *op = label;
        }
        if (labelMask) {                       // (uniform) the word of the pixels whose label moved: an OR over wave 0
            unsigned lo32 = (unsigned)moved, hi32 = (unsigned)(moved >> 32);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                lo32 |= (unsigned)__shfl_xor((int)lo32, o);
                hi32 |= (unsigned)__shfl_xor((int)hi32, o);
            }
            if (threadIdx.x == 0) labelMask[w] = ((unsigned long long)hi32 << 32) | lo32;
        }
    } else if (writer) {
        float S = 0.f, Q = 0.f;
        if (SUMS) {
            float p[NP], p2[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                p[i] = __uint_as_float(red[rows::SUM][i * PX + px]);
                p2[i] = __uint_as_float(red[rows::SQ][i * PX + px]);
            }
            S = cbc_tree<NP>(p);
            Q = cbc_tree<NP>(p2);
        }
        if (EXT)
#pragma unroll
            for (int i = 0; i < NP; ++i) L = cbc_better(L, cbc_read<true>(red, rows::LO, i * PX + px));
        T* op = (T*)out + first + bit;
#pragma clang loop vectorize(disable) unroll(disable)
        for (int k = 0; k < nOps; ++k) {       // channel k of `out` for op k
            const int kind = (ops >> (4 * k)) & 15;
            const float y = kind == CB_CC_SUM    ? S
                            : kind == CB_CC_MEAN ? S / (float)C
                            : kind == CB_CC_NORM ? sqrtf(Q)
                            : kind == CB_CC_MAX  ? H.v
                                                 : L.v;      // (the value AT the index: -0 where -0 comes first)
            op[(long)k * HW] = (T)y;
        }
    }
}

// x [C, H, W]; out [nOps, H, W] of T, or (CBC_ARG) [H, W] int64.  mask: the operand's change mask of this frame, or
// NULL; all: every pixel is listed.  An operand without a mask has its bits in `bits` already (list form) -- or did not
// change.  labelMask (CBC_ARG only, or NULL): every word is written, a bit set where a listed pixel's label moved.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void cbc_chancollapse_kernel(const T* __restrict__ x, void* __restrict__ out,
                                                              const unsigned long long* __restrict__ mask, int all,
                                                              unsigned long long* bits,
                                                              unsigned long long* __restrict__ maskCopy,
                                                              unsigned long long* __restrict__ labelMask, long words,
                                                              int C, int H, int W, int wpr, int ops, int nOps) {
    __shared__ unsigned red[2][cbc_rows<MODE>::N][256];
    const long HW = (long)H * W;
    unsigned turn = 0;
    cb_walk_word_units(
        bits, maskCopy, words, W, wpr, all,
        [&](long w, int, int) {
            // (an empty word's label mask is zero; thread 0 also stores a non-empty word's, afterwards)
            if (MODE == CBC_ARG && labelMask && threadIdx.x == 0) labelMask[w] = 0ull;
            return mask ? mask[w] : 0ull;
        },
        [&](unsigned long long word, int y, int tile) {
            const int n = __popcll(word);
            const long first = (long)y * W + tile * 64;      // (H W fits an int: cbc_args_ok)
            const long w = (long)y * wpr + tile;
            unsigned(*r)[256] = red[turn++ & 1u];
            // (the word is uniform over the workgroup, and so is the barrier of either form)
            if (n > 16)
                cbc_word<T, MODE, 4>(x, out, labelMask, w, all, word, n, first, HW, C, ops, nOps, r);
            else
                cbc_word<T, MODE, 1>(x, out, labelMask, w, all, word, n, first, HW, C, ops, nOps, r);
        });
}

template <typename T>
void cbc_launch(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits, uint64_t* maskCopy,
                uint64_t* labelMask, int C, int H, int W, int ops, int nOps, hipStream_t s) {
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
    const int mode = cbc_mode(ops, nOps);
#define CBC_GO(MODE)                                                                                                \
    if (mode == MODE)                                                                                               \
    hipLaunchKernelGGL((cbc_chancollapse_kernel<T, MODE>), grid, block, 0, s, (const T*)x, out,                     \
                       (const unsigned long long*)mask, all, (unsigned long long*)bits, (unsigned long long*)maskCopy, \
                       (unsigned long long*)labelMask, words, C, H, W, wpr, ops, nOps)
    CBC_GO(CBC_ARG);
    CBC_GO(CBC_SUMS);
    CBC_GO(CBC_EXTREMES);
    CBC_GO(CBC_BOTH);
#undef CBC_GO
}

// what both entry points ask of the tensors, the module's masks and the kinds
bool cbc_args_ok(const void* x, const void* out, const uint64_t* mask, const uint64_t* bits, const uint64_t* maskCopy,
                 const uint64_t* labelMask, int C, int H, int W, int ops, int nOps, int dtype) {
    return x && out && x != out && bits && maskCopy && bits != maskCopy && mask != bits && mask != maskCopy && H >= 1 &&
           W >= 1 && (dtype == CB_F32 || dtype == CB_F16) && cbinfer_chancollapse_supported(ops, nOps, C) &&
           (!labelMask || (cbc_kind(ops, 0) >= CB_CC_ARGMAX && labelMask != bits && labelMask != maskCopy &&
                           labelMask != mask && (const void*)labelMask != x && (const void*)labelMask != out)) &&
           // (a list addresses a pixel with an int32; 64 C as for the other mask-driven operators)
           (long)H * W < (1l << 31) && (long)C * 64 < (1l << 31);
}

}  // namespace

int cbinfer_chancollapse_supported(int ops, int nOps, int C) {
    if (nOps < 1 || nOps > 4 || C < 1 || ops < 0 || (ops >> (4 * nOps)) != 0) return 0;
    for (int k = 0; k < nOps; ++k) {
        const int kind = cbc_kind(ops, k);
        if (kind > CB_CC_ARGMIN || (kind >= CB_CC_ARGMAX && nOps != 1)) return 0;
    }
    return 1;
}

int cbinfer_chancollapse_changed(const void* x, void* out, const uint64_t* mask, int all, uint64_t* bits,
                                 uint64_t* maskCopy, uint64_t* labelMask, int C, int H, int W, int ops, int nOps,
                                 int dtype, cbStream_t stream) {
    CB_REQUIRE(cbc_args_ok(x, out, mask, bits, maskCopy, labelMask, C, H, W, ops, nOps, dtype));
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbc_launch<decltype(t)>(x, out, mask, all, bits, maskCopy, labelMask, C, H, W, ops, nOps, (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbchancollapse_forward(const void* x, void* outputState, const uint64_t* mask, const int32_t* list, int capN,
                                   const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, uint64_t* labelMask, int C,
                                   int H, int W, int ops, int nOps, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(cbc_args_ok(x, outputState, mask, bits, maskCopy, labelMask, C, H, W, ops, nOps, dtype));
    CB_REQUIRE(capN >= 0 && !(mask && list) && (list || !countDev));
    if (list) {
        const int st = cb_list_to_bits(list, capN, countDev, H, W, bits, stream);
        if (st != CB_OK) return st;
    }
    return cbinfer_chancollapse_changed(x, outputState, mask, !mask && !list, bits, maskCopy, labelMask, C, H, W, ops,
                                        nOps, dtype, stream);
}
