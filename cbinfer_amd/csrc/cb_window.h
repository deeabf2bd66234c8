// What the two window operators of two maps share (cb_corr.hip: the correlation layer; cb_aggr.hip: the
// per-pixel kernel application): the limits of a displacement window, the footprint word of the frame
// launch's mask walk, the argument checks of the two operands' forms, the list-form launches in front of the frame and
// the clearing launch behind it.  In both operators operand A (`a` / `w`) is read at the pixel itself and operand B
// (`b` / `v`) at the window's taps.
#pragma once
#include "cb_maskwalk.h"

#define CBW_MAXDISP 64
#define CBW_MAXSTEP 8
#define CBW_MAXTAPS 512

// the displacements y0 + i step, i < Dy, and x0 + j step, j < Dx
struct cbw_window {
    int y0, x0, step, Dy, Dx;
};

// The word of the frame's mask for row y, word `tile`: A's mask word ORed with the windows of B's mask at every
// displacement -- the (i, j) shifts dealt over the 64 lanes of every wave, two 64-bit loads and a funnel shift each,
// OR-reduced by a butterfly: every wave makes the same word.  maskA: A's change mask of this frame, or NULL (a list is
// in the working mask already); maskB: B's -- its own, or the working mask its list went into --, or NULL: B did not
// change (uniform over the workgroup).
__device__ __forceinline__ unsigned long long cbw_footprint_word(const unsigned long long* __restrict__ maskA,
                                                                 const unsigned long long* __restrict__ maskB, long w,
                                                                 int y, int tile, int H, int wpr, const cbw_window& g,
                                                                 int lane) {
    unsigned long long word = maskA ? maskA[w] : 0ull;
    if (maskB) {
        unsigned long long m = 0ull;
        const int shifts = g.Dy * g.Dx;
        for (int e = lane; e < shifts; e += 64) {
            const int i = e / g.Dx, j = e - i * g.Dx;
            const int yy = y + g.y0 + i * g.step;
            if (yy < 0 || yy >= H) continue;
            // the 64 bits of B's mask row yy from column xs on: bit x' is the tap of pixel 64 tile + x'
            const int xs = tile * 64 + g.x0 + j * g.step;      // (>= -64)
            const int wi = xs >> 6, sh = xs & 63;
            const unsigned long long* row = maskB + (long)yy * wpr;
            const unsigned long long lo = (wi >= 0 && wi < wpr) ? row[wi] : 0ull;
            const unsigned long long hi = (sh != 0 && wi + 1 >= 0 && wi + 1 < wpr) ? row[wi + 1] : 0ull;
            m |= (lo >> sh) | (sh != 0 ? hi << (64 - sh) : 0ull);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m |= __shfl_xor(m, o);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
        word |= ((unsigned long long)hi << 32) | lo;
    }
    return word;
}

// behind a frame whose B came as a list: zero to the words of B's working mask that the list named (plain stores of
// one value: entries that share a word do not matter)
static __global__ __launch_bounds__(256) void cbw_clear_list_kernel(const int32_t* __restrict__ list, int nHost,
                                                                   const int32_t* __restrict__ countDev, int H, int W,
                                                                   int wpr, unsigned long long* __restrict__ bBits) {
    const int N = countDev ? min(*countDev, nHost) : nHost;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        const int pos = list[i];
        if ((unsigned)pos >= (unsigned)(H * W)) continue;      // (an out-of-map entry set no bit)
        const int y = pos / W, x = pos - y * W;
        bBits[(long)y * wpr + (x >> 6)] = 0ull;
    }
}

inline bool cbw_range_ok(int lo, int hi, int step) {
    return lo >= -CBW_MAXDISP && hi <= CBW_MAXDISP && lo <= hi && (hi - lo) % step == 0;
}

// the limits of a window: both ranges, the step, Dy Dx <= CBW_MAXTAPS
inline bool cbw_window_ok(int y0, int y1, int x0, int x1, int step) {
    if (!(step >= 1 && step <= CBW_MAXSTEP && cbw_range_ok(y0, y1, step) && cbw_range_ok(x0, x1, step))) return false;
    return ((y1 - y0) / step + 1) * ((x1 - x0) / step + 1) <= CBW_MAXTAPS;
}

// the two operands' forms and the three mask buffers, as the entry points take them
struct cbw_forms {
    const uint64_t* maskA;
    const int32_t* listA;
    int capA;
    const int32_t* countA;
    const uint64_t* maskB;
    const int32_t* listB;
    int capB;
    const int32_t* countB;
    uint64_t *bBits, *bits, *maskCopy;
};

inline bool cbw_forms_ok(const cbw_forms& f) {
    return f.bBits && f.bits && f.maskCopy && f.bBits != f.bits && f.bBits != f.maskCopy && f.bits != f.maskCopy &&
           f.capA >= 0 && !(f.maskA && f.listA) && (f.listA || !f.countA) &&
           f.capB >= 0 && !(f.maskB && f.listB) && (f.listB || !f.countB) &&
           f.maskA != f.bBits && f.maskA != f.bits && f.maskA != f.maskCopy &&
           f.maskB != f.bBits && f.maskB != f.bits && f.maskB != f.maskCopy;
}

// what the frame launch is handed
struct cbw_frame {
    int all;                    // every pixel is listed, neither mask is read
    bool bList;                 // B's list went into bBits: the clearing launch follows the frame
    const uint64_t *mA, *mB;
};

// The launches in front of the frame: A's list into `bits`, B's into `bBits`.  An operand with neither mask nor list
// lists every pixel: the other's changes are not needed then.
inline int cbw_lists_to_bits(const cbw_forms& f, int H, int W, cbStream_t stream, cbw_frame* fr) {
    fr->all = (!f.maskA && !f.listA) || (!f.maskB && !f.listB);
    fr->bList = !fr->all && f.listB && f.capB > 0;
    if (!fr->all && f.listA) {
        const int st = cb_list_to_bits(f.listA, f.capA, f.countA, H, W, f.bits, stream);
        if (st != CB_OK) return st;
    }
    if (fr->bList) {
        const int st = cb_list_to_bits(f.listB, f.capB, f.countB, H, W, f.bBits, stream);
        if (st != CB_OK) return st;
    }
    fr->mA = fr->all ? nullptr : f.maskA;
    fr->mB = fr->all ? nullptr : (f.maskB ? f.maskB : (fr->bList ? f.bBits : nullptr));
    return CB_OK;
}

// The launch behind the frame (the frame launch reads B's mask from every workgroup, so it cannot clear it itself).
inline int cbw_clear_list(const cbw_forms& f, int H, int W, hipStream_t s) {
    long blocks = ((long)f.capB + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(cbw_clear_list_kernel, dim3((unsigned)blocks), dim3(256), 0, s, f.listB, f.capB, f.countB, H, W,
                       (W + 63) / 64, (unsigned long long*)f.bBits);
    return cb_launch_status();
}
