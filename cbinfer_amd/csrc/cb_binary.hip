// Change-based element-wise operators of two maps -- sum, difference, product (plain or gated: a * sigmoid(b),
// a * hardsigmoid(b)), maximum and minimum -- on gfx950.  The reference has no such operator; contracts of
// the entry points and the arithmetic in include/cbinfer_hip.h.  Every producer of this library leaves the pixels outside
// its change list bit for bit as they were, so op(a, b) can differ from last frame's only at the UNION of the two
// operands' changes -- and a constant operand never changes --: recomputing there gives the dense result exactly,
// without a threshold.  A frame is
//   per operand in LIST form, one launch in front: the list's bits ORed into the zeroed working mask
//              (cb_list_to_bits of cb_maskwalk.h);
//   one launch, the word walk of cb_maskwalk.h: the operands' change masks (or the full row word of an operand without
//              change information) are ORed into the working word, one value per (set bit, channel).
// The second operand is addressed as b[c sc + p sp], which covers a map, a one-channel map, a channel vector and a
// scalar with ONE kernel; only the one-channel map (CB_BIN_PIXEL) has a kernel of its own, since there the operand --
// with its gate, an expf -- belongs to the pixel and not to the (pixel, channel) item: it is evaluated once per set bit
// of the word into LDS and shared over the channels (cb_walk_word_units).  No host sync, memset, allocation, data
// atomics or inline assembly.
#include "cb_maskwalk.h"

// (no multiply-add is ever formed here; the pragma keeps v + 3 and the division of the hard sigmoid as written)
#pragma clang fp contract(off)

namespace {

// what a launch computes: op, gate and reverse folded into one template parameter (gates exist for the product only,
// reverse for the difference only)
enum { CBB_ADD, CBB_SUB, CBB_RSUB, CBB_MUL, CBB_MUL_SIGMOID, CBB_MUL_HARDSIGMOID, CBB_MAXIMUM, CBB_MINIMUM };

inline int cbb_function(int op, int gate, int reverse) {
    switch (op) {
        case CB_BIN_ADD: return CBB_ADD;
        case CB_BIN_SUB: return reverse ? CBB_RSUB : CBB_SUB;
        case CB_BIN_MUL:
            return gate == CB_BIN_GATE_SIGMOID ? CBB_MUL_SIGMOID
                                               : (gate == CB_BIN_GATE_HARDSIGMOID ? CBB_MUL_HARDSIGMOID : CBB_MUL);
        case CB_BIN_MAXIMUM: return CBB_MAXIMUM;
        default: return CBB_MINIMUM;
    }
}

// The second operand as the operation takes it: g(b) in f32, rounded to the operand dtype as the separate torch operator
// would round it (the formulas are cb_pointwise.hip's; comparisons, so a NaN stays a NaN); b itself without a gate.
template <typename T, int FN>
__device__ __forceinline__ float cbb_operand(float b) {
    if (FN == CBB_MUL_SIGMOID) return (float)(T)(1.f / (1.f + expf(-b)));
    if (FN == CBB_MUL_HARDSIGMOID) {
        const float t = b + 3.f;
        return (float)(T)((t < 0.f ? 0.f : (t > 6.f ? 6.f : t)) / 6.f);
    }
    return b;
}

// One correctly rounded f32 operation.  Maximum / minimum by comparisons: a NaN if either operand is one, and `a` on a
// tie (+0 against -0 included).
template <int FN>
__device__ __forceinline__ float cbb_apply(float a, float b) {
    switch (FN) {
        case CBB_ADD: return a + b;
        case CBB_SUB: return a - b;
        case CBB_RSUB: return b - a;
        case CBB_MAXIMUM: return a != a ? a : (b != b ? b : (b > a ? b : a));
        case CBB_MINIMUM: return a != a ? a : (b != b ? b : (b < a ? b : a));
        default: return a * b;
    }
}

// a, out [C, H, W]; b addressed as b[c sc + p sp], p = y W + x.  maskA / maskB: the operand's change mask of this frame,
// or NULL; all: one of the operands lists every pixel.  An operand without a mask has its bits in `bits` already (list
// form) -- or did not change.  PIXEL: sc == 0, sp == 1; a word's operand values are staged in LDS by the threads of the
// first wave, one per set bit, into one of two regions used in turn -- a word's items read theirs behind ONE barrier,
// and the region is written again only behind the barrier of the word after.  The region holds the operand dtype, in
// which the values are exact: an f16 product then has two f16 operands, as in the other forms.  (Held as f32, hipcc
// forms the f16 product as v_fma_mixlo_f16 with an addend of +0, which loses the sign of a zero product.)
template <typename T, int FN, bool PIXEL>
__global__ __launch_bounds__(256) void cbb_binary_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                        T* __restrict__ out, const unsigned long long* __restrict__ maskA,
                                                        const unsigned long long* __restrict__ maskB, int all,
                                                        unsigned long long* bits,
                                                        unsigned long long* __restrict__ maskCopy, long words, int C,
                                                        int H, int W, int wpr, long sc, int sp) {
    __shared__ T shared[2 * 64];
    const long HW = (long)H * W;
    auto makeWord = [&](long w, int, int) { return (maskA ? maskA[w] : 0ull) | (maskB ? maskB[w] : 0ull); };
    if (PIXEL) {
        unsigned turn = 0;
        cb_walk_word_units(bits, maskCopy, words, W, wpr, all, makeWord, [&](unsigned long long word, int y, int tile) {
            T* g = shared + (turn++ & 1u) * 64;
            const long first = (long)y * W + tile * 64;      // (H W fits an int: cbb_args_ok)
            // (a set bit is a pixel of the row: cb_valid_mask)
            if (threadIdx.x < 64 && ((word >> threadIdx.x) & 1ull))
                g[threadIdx.x] = (T)cbb_operand<T, FN>(cb_load_f32(b + first + threadIdx.x));      // (exact)
            __syncthreads();      // (the word is uniform over the workgroup)
            cb_walk_items(word, C, [&](int c, int bit) {
                const long o = (long)c * HW + first + bit;
                out[o] = (T)cbb_apply<FN>(cb_load_f32(a + o), cb_load_f32(g + bit));      // fp16: rounded once
            });
        });
    } else {
        cb_walk_words(bits, maskCopy, words, C, W, wpr, all, makeWord, [&](int c, int y, int x) {
            const long p = (long)y * W + x;
            const long o = (long)c * HW + p;
            const float bv = cbb_operand<T, FN>(cb_load_f32(b + (c * sc + p * sp)));
            out[o] = (T)cbb_apply<FN>(cb_load_f32(a + o), bv);      // fp16: rounded once
        });
    }
}

template <typename T>
void cbb_launch(const void* a, const void* b, void* out, const uint64_t* maskA, const uint64_t* maskB, int all,
                uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int bForm, int fn, hipStream_t s) {
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr, HW = (long)H * W;
    const dim3 grid(cb_walk_grid(words)), block(256);
    const bool perChannel = bForm == CB_BIN_MAP || bForm == CB_BIN_HALVES || bForm == CB_BIN_CHANNEL;
    const bool perPixel = bForm == CB_BIN_MAP || bForm == CB_BIN_HALVES || bForm == CB_BIN_PIXEL;
    const long sc = !perChannel ? 0 : (perPixel ? HW : 1);
    const int sp = perPixel ? 1 : 0;
#define CBB_GO(FN, PIXEL)                                                                                             \
    hipLaunchKernelGGL((cbb_binary_kernel<T, FN, PIXEL>), grid, block, 0, s, (const T*)a, (const T*)b, (T*)out,       \
                       (const unsigned long long*)maskA, (const unsigned long long*)maskB, all,                      \
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, C, H, W, wpr, sc, sp)
#define CBB_FN(FN)              \
    case FN:                    \
        if (bForm == CB_BIN_PIXEL) \
            CBB_GO(FN, true);   \
        else                    \
            CBB_GO(FN, false);  \
        break
    switch (fn) {
        CBB_FN(CBB_ADD);
        CBB_FN(CBB_SUB);
        CBB_FN(CBB_RSUB);
        CBB_FN(CBB_MUL);
        CBB_FN(CBB_MUL_SIGMOID);
        CBB_FN(CBB_MUL_HARDSIGMOID);
        CBB_FN(CBB_MAXIMUM);
        CBB_FN(CBB_MINIMUM);
    }
#undef CBB_FN
#undef CBB_GO
}

// The second operand's address: the upper half of `a` ([2C, H, W]) in CB_BIN_HALVES form, where none is given.
const void* cbb_second(const void* a, const void* b, int C, int H, int W, int bForm, int dtype) {
    if (bForm != CB_BIN_HALVES) return b;
    return (const char*)a + (long)C * H * W * (dtype == CB_F32 ? 4 : 2);
}

// what both entry points ask of the tensors, the module's two masks, the operand form and the function
bool cbb_args_ok(const void* a, const void* b, const void* out, const uint64_t* maskA, const uint64_t* maskB,
                 const uint64_t* bits, const uint64_t* maskCopy, int C, int H, int W, int bForm, int op, int gate,
                 int reverse, int dtype) {
    if (!(a && out && bits && maskCopy && bits != maskCopy && C >= 1 && H >= 1 && W >= 1 &&
          (dtype == CB_F32 || dtype == CB_F16) && bForm >= CB_BIN_MAP && bForm <= CB_BIN_HALVES &&
          cbinfer_binary_supported(op, gate, reverse) &&
          // (a list addresses a pixel with an int32; the kernel numbers a word's items with an int)
          (long)H * W < (1l << 31) && (long)C * 64 < (1l << 31)))
        return false;
    if (bForm == CB_BIN_HALVES ? b != nullptr : b == nullptr) return false;
    // (only a map or a one-channel map has changed pixels of its own)
    if (maskB && bForm != CB_BIN_MAP && bForm != CB_BIN_PIXEL) return false;
    return out != a && out != cbb_second(a, b, C, H, W, bForm, dtype) && maskA != maskCopy && maskB != maskCopy &&
           maskA != bits && maskB != bits;
}

}  // namespace

int cbinfer_binary_supported(int op, int gate, int reverse) {
    if (op < CB_BIN_ADD || op > CB_BIN_MINIMUM) return 0;
    if (gate < CB_BIN_GATE_NONE || gate > CB_BIN_GATE_HARDSIGMOID) return 0;
    if (gate != CB_BIN_GATE_NONE && op != CB_BIN_MUL) return 0;
    if (reverse && op != CB_BIN_SUB) return 0;
    return 1;
}

int cbinfer_binary_changed(const void* a, const void* b, void* out, const uint64_t* maskA, int allA, const uint64_t* maskB,
                           int allB, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int bForm, int op, int gate,
                           int reverse, int dtype, cbStream_t stream) {
    CB_REQUIRE(cbb_args_ok(a, b, out, maskA, maskB, bits, maskCopy, C, H, W, bForm, op, gate, reverse, dtype));
    const int all = allA || allB;
    const void* second = cbb_second(a, b, C, H, W, bForm, dtype);
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbb_launch<decltype(t)>(a, second, out, maskA, maskB, all, bits, maskCopy, C, H, W, bForm,
                                cbb_function(op, gate, reverse), (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbbinary_forward(const void* a, const void* b, void* outputState, const uint64_t* maskA, const int32_t* listA,
                             int capA, const int32_t* countA, const uint64_t* maskB, const int32_t* listB, int capB,
                             const int32_t* countB, int bForm, int bChanges, uint64_t* bits, uint64_t* maskCopy, int C,
                             int H, int W, int op, int gate, int reverse, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(cbb_args_ok(a, b, outputState, maskA, maskB, bits, maskCopy, C, H, W, bForm, op, gate, reverse, dtype));
    CB_REQUIRE(bChanges == CB_BIN_B_NONE || bChanges == CB_BIN_B_OWN);
    CB_REQUIRE(capA >= 0 && capB >= 0);
    CB_REQUIRE(!(maskA && listA) && !(maskB && listB));
    CB_REQUIRE((listA || !countA) && (listB || !countB));
    const bool bHasPixels = bForm == CB_BIN_MAP || bForm == CB_BIN_PIXEL;
    // an operand that contributes no pixel takes neither mask nor list; the upper half of `a` changes with `a`
    CB_REQUIRE(!((maskB || listB) && (!bHasPixels || bChanges == CB_BIN_B_NONE)));
    CB_REQUIRE(!(bForm == CB_BIN_HALVES && bChanges == CB_BIN_B_OWN));
    const int allA = !maskA && !listA;
    // (a per-frame channel vector or scalar changes the whole map)
    const int allB = bChanges == CB_BIN_B_OWN && !maskB && !listB;
    if (!allA && !allB) {      // (behind an operand that lists every pixel the other's list changes nothing)
        int st = CB_OK;
        if (listA) st = cb_list_to_bits(listA, capA, countA, H, W, bits, stream);
        if (st == CB_OK && listB) st = cb_list_to_bits(listB, capB, countB, H, W, bits, stream);
        if (st != CB_OK) return st;
    }
    return cbinfer_binary_changed(a, b, outputState, maskA, allA, maskB, allB, bits, maskCopy, C, H, W, bForm, op, gate,
                                  reverse, dtype, stream);
}
