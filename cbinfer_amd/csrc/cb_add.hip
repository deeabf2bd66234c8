// Change-based element-wise sum of two maps, out = a + b [then ReLU], on gfx950.  The reference has no
// such operator; contracts of the entry points in include/cbinfer_hip.h.  Every producer of this library leaves the
// pixels outside its change list bit for bit as they were, so the sum can differ from last frame's only at the UNION of
// the two operands' changes: recomputing there gives the dense result exactly, without a threshold.  A frame is
//   per operand in LIST form, one launch in front: the list's bits ORed into the zeroed working mask
//              (cb_list_to_bits of cb_maskwalk.h);
//   one launch, the word walk of cb_maskwalk.h (cb_walk_words): the operands' change masks (or the full row word of
//              an operand without change information) are ORed into the working word, one sum per (set bit, channel).
// No host sync, memset, allocation, data atomics or inline assembly.
#include "cb_maskwalk.h"

namespace {

// a, b, out [C, H, W].  maskA / maskB: the operand's change mask of this frame, or NULL; all: one of the operands lists
// every pixel.  An operand without a mask has its bits in `bits` already (list form) -- or did not change.
template <typename T, int RELU>
__global__ __launch_bounds__(256) void cba_add_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                     T* __restrict__ out, const unsigned long long* __restrict__ maskA,
                                                     const unsigned long long* __restrict__ maskB, int all,
                                                     unsigned long long* bits, unsigned long long* __restrict__ maskCopy,
                                                     long words, int C, int H, int W, int wpr) {
    const long HW = (long)H * W;
    cb_walk_words(
        bits, maskCopy, words, C, W, wpr, all,
        [&](long w, int, int) { return (maskA ? maskA[w] : 0ull) | (maskB ? maskB[w] : 0ull); },
        [&](int c, int y, int x) {
            const long o = (long)c * HW + (y * W + x);      // (H W fits an int: cba_args_ok)
            // fp32: one IEEE addition; fp16: the sum in f32, rounded to f16 once (the correctly rounded f16 sum)
            float v = cb_load_f32(a + o) + cb_load_f32(b + o);
            if (RELU) v = v != v ? v : (v > 0.f ? v : 0.f);      // (a NaN stays a NaN, as torch.relu)
            out[o] = (T)v;
        });
}

template <typename T>
void cba_launch(const void* a, const void* b, void* out, const uint64_t* maskA, const uint64_t* maskB, int all,
                uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int relu, hipStream_t s) {
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBA_GO(RELU)                                                                                                  \
    hipLaunchKernelGGL((cba_add_kernel<T, RELU>), grid, block, 0, s, (const T*)a, (const T*)b, (T*)out,              \
                       (const unsigned long long*)maskA, (const unsigned long long*)maskB, all,                      \
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, C, H, W, wpr)
    if (relu)
        CBA_GO(1);
    else
        CBA_GO(0);
#undef CBA_GO
}

// what both entry points ask of the tensors and the two masks of the module
bool cba_args_ok(const void* a, const void* b, const void* out, const uint64_t* bits, const uint64_t* maskCopy, int C, int H,
                 int W, int dtype) {
    return a && b && out && bits && maskCopy && bits != maskCopy && C >= 1 && H >= 1 && W >= 1 &&
           (dtype == CB_F32 || dtype == CB_F16) &&
           // (a list addresses a pixel with an int32; the kernel numbers a word's items with an int)
           (long)H * W < (1l << 31) && (long)C * 64 < (1l << 31);
}

}  // namespace

int cbinfer_add_changed(const void* a, const void* b, void* out, const uint64_t* maskA, int allA, const uint64_t* maskB,
                        int allB, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int relu, int dtype,
                        cbStream_t stream) {
    CB_REQUIRE(cba_args_ok(a, b, out, bits, maskCopy, C, H, W, dtype));
    CB_REQUIRE(maskA != maskCopy && maskB != maskCopy && maskA != bits && maskB != bits);
    const int all = allA || allB;
    cb_dispatch_dtype(dtype, [&](auto t) {
        cba_launch<decltype(t)>(a, b, out, maskA, maskB, all, bits, maskCopy, C, H, W, relu, (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbadd_forward(const void* a, const void* b, void* outputState, const uint64_t* maskA, const int32_t* listA,
                          int capA, const int32_t* countA, const uint64_t* maskB, const int32_t* listB, int capB,
                          const int32_t* countB, uint64_t* bits, uint64_t* maskCopy, int C, int H, int W, int relu,
                          int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(cba_args_ok(a, b, outputState, bits, maskCopy, C, H, W, dtype));
    CB_REQUIRE(capA >= 0 && capB >= 0);
    CB_REQUIRE(!(maskA && listA) && !(maskB && listB));
    CB_REQUIRE((listA || !countA) && (listB || !countB));
    CB_REQUIRE(maskA != maskCopy && maskB != maskCopy && maskA != bits && maskB != bits);
    const int allA = !maskA && !listA, allB = !maskB && !listB;
    if (!allA && !allB) {      // (behind an operand that lists every pixel the other's list changes nothing)
        int st = CB_OK;
        if (listA) st = cb_list_to_bits(listA, capA, countA, H, W, bits, stream);
        if (st == CB_OK && listB) st = cb_list_to_bits(listB, capB, countB, H, W, bits, stream);
        if (st != CB_OK) return st;
    }
    return cbinfer_add_changed(a, b, outputState, maskA, allA, maskB, allB, bits, maskCopy, C, H, W, relu, dtype, stream);
}
