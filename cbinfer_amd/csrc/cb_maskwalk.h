// What the mask-driven element-wise operators share (cb_add.hip, cb_pointwise.hip, cb_decoder.hip, cb_pool2d.hip,
// cb_dwconv.hip, cb_adaptpool.hip): the walk over the words of a working mask, its item loop, the grid sizing, the f32 load
// of either dtype, the list -> working mask launch and the dtype dispatch of the entry points.
#pragma once
#include "cb_common.h"

// one value of either dtype as f32 (exact)
__device__ __forceinline__ float cb_load_f32(const float* p) { return *p; }
__device__ __forceinline__ float cb_load_f32(const cb_half* p) { return (float)*p; }

// The (set bit, channel) items of a non-empty mask word spread over the 256 threads of the workgroup, set bit fastest:
// item(c, bit) with bit the position in the word, c < C.
template <typename Item>
__device__ __forceinline__ void cb_walk_items(unsigned long long word, int C, Item item) {
    const int n = __popcll(word);
    const int total = n * C;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int c = e / n, i = e - c * n;
        item(c, n == 64 ? i : cb_select_bit(word, i));
    }
}

// The walk: workgroups of four waves stride over the `words` words of `bits`, the working mask of a W-wide map with
// wpr words per row (zero between frames; an operand in list form has its bits there already).  Per word w of row y:
//   word = bits[w] | makeWord(w, y, tile), cut to the pixels of the row -- or, with all != 0, every pixel of the row;
//   thread 0 stores it to maskCopy[w], the frame's mask;
//   item(c, y, x) for every set bit -- pixel (y, x) of the map -- and c < C (cb_walk_items);
//   a working word that was not zero is zeroed behind a barrier, for the next frame.
// makeWord runs on all 256 threads and must return the same value on each of them (it may hold a ballot: every wave
// makes the same word); it is also called for a word whose result `all` replaces, so it may prepare what item reads.
template <typename MakeWord, typename Item>
__device__ __forceinline__ void cb_walk_words(unsigned long long* bits, unsigned long long* __restrict__ maskCopy,
                                              long words, int C, int W, int wpr, int all, MakeWord makeWord, Item item) {
    for (long w = blockIdx.x; w < words; w += gridDim.x) {
        // (uniform over the workgroup: the working word is zeroed only behind the barrier below)
        const unsigned long long own = bits[w];
        const int y = (int)(w / wpr), tile = (int)(w - (long)y * wpr);
        const unsigned long long valid = cb_valid_mask(W, tile);
        unsigned long long word = own | makeWord(w, y, tile);
        word = all ? valid : (word & valid);      // (the bits of the row padding are never set)
        if (threadIdx.x == 0) maskCopy[w] = word;
        if (word != 0) cb_walk_items(word, C, [&](int c, int bit) { item(c, y, tile * 64 + bit); });
        if (own != 0) {
            __syncthreads();      // every wave has read the word
            if (threadIdx.x == 0) bits[w] = 0;
        }
    }
}

// The same walk for an operator whose unit of work is the whole word (cb_chanreduce.hip: a reduction over the channels
// of each listed pixel, which the (set bit, channel) items of cb_walk_items cannot express): the same OR of working
// word and makeWord, the same cut, maskCopy store and zeroing; unit(word, y, tile) runs on all 256 threads for every
// non-empty word, which is uniform over the workgroup -- unit may hold barriers.
template <typename MakeWord, typename Unit>
__device__ __forceinline__ void cb_walk_word_units(unsigned long long* bits, unsigned long long* __restrict__ maskCopy,
                                                   long words, int W, int wpr, int all, MakeWord makeWord, Unit unit) {
    for (long w = blockIdx.x; w < words; w += gridDim.x) {
        const unsigned long long own = bits[w];
        const int y = (int)(w / wpr), tile = (int)(w - (long)y * wpr);
        const unsigned long long valid = cb_valid_mask(W, tile);
        unsigned long long word = own | makeWord(w, y, tile);
        word = all ? valid : (word & valid);      // (the bits of the row padding are never set)
        if (threadIdx.x == 0) maskCopy[w] = word;
        if (word != 0) unit(word, y, tile);
        if (own != 0) {
            __syncthreads();      // every wave has read the word
            if (threadIdx.x == 0) bits[w] = 0;
        }
    }
}

// workgroups of a persistent grid over `units` units of work: all of them, at most eight per CU
inline unsigned cb_walk_grid(long units) {
    const long cap = (long)cb_num_cus() * 8;
    return (unsigned)(units < cap ? units : cap);
}

// One launch: the pixels of a change list ORed into the zeroed working mask `bits` of their own H x W map
// (cbinfer_pool_footprint of cb_pool2d.hip with a 1x1 / stride-1 window, which reaches its own pixel only: one 64-bit
// atomicOr per entry; cap == 0 launches nothing).
inline int cb_list_to_bits(const int32_t* list, int cap, const int32_t* count, int H, int W, uint64_t* bits,
                           cbStream_t stream) {
    const cbPool one = {1, 1, 1, 1, 0, 0, 0, CB_POOL_MAX};
    return cbinfer_pool_footprint(list, cap, count, nullptr, H, W, &one, bits, stream);
}

// f(T()) with T the element type of `dtype` (CB_F32, else CB_F16: the entry points have checked it)
template <typename F>
inline void cb_dispatch_dtype(int dtype, F f) {
    if (dtype == CB_F32)
        f(float());
    else
        f(cb_half());
}
