// What the gather contractions share (cb_geomconv.hip, cb_tconv.hip, cb_groupconv.hip), written once:
//   host    tile constants, workspace layout, the list / mask arguments of an entry point, the state protocol of a frame
//           entry point, the arithmetic dispatch, the detection launch;
//   device  the detection kernels' channel scan, the tap-table entry, the mask -> list prologue and the list lookup, the
//           weight-row load and the 8-tap gather of a stage, the LDS stage images and -- for the 64 x 64 x 32 tile of
//           cbg_conv_kernel and cbt_conv_kernel -- the MFMA stage, the stage pipeline, the split-k hand-off and the
//           epilogue.  Functions where the kernels' disassembly stays the parent's, statement macros where it does not
//           (CBG_LIST_COUNT, CBG_GATHER8, CBG_TILE_STAGES, CBG_SPLITK_HANDOFF, CBG_TILE_STORE).
#pragma once
#include "cb_common.h"

namespace {

typedef unsigned short ushortx8 __attribute__((ext_vector_type(8)));

#define CBG_BM 64        // output channels per tile
#define CBG_BN 64        // listed pixels per tile
#define CBG_BK 32        // k-depth per LDS stage
#define CBG_GRID 512     // persistent grid of the contractions (2 workgroups per CU of an MI355X)
#define CBG_SKMAX 8      // most k-slices per tile
#define CBG_SLAB (CBG_BM * CBG_BN)
#define CBG_ROW16 40      // LDS row of 32 16-bit k-slots + 16 bytes (16-byte fragment reads free of conflicts)
#define CBG_ROW32 33

inline int cbg_kpad(int K) { return (K + CBG_BM - 1) / CBG_BM * CBG_BM; }
inline int cbg_ckkpad(int Ckk) { return (Ckk + CBG_BK - 1) / CBG_BK * CBG_BK; }

// ---------------------------------------------------------------------------------------------
// host side of the entry points
// ---------------------------------------------------------------------------------------------
// split-k workspace: one slab per workgroup of the grid, then the arrival counters (zero between launches)
struct CbgWorkspace {
    float* slabs;      // null: no split
    int* tickets;
};
inline long cbg_workspace_bytes() { return (long)CBG_GRID * CBG_SLAB * 4 + (long)CBG_GRID * 4; }
inline CbgWorkspace cbg_workspace(void* workspace) {
    CbgWorkspace w = {};
    if (workspace) w = {(float*)workspace, (int*)((char*)workspace + (long)CBG_GRID * CBG_SLAB * 4)};
    return w;
}

// the listed pixels of a contraction launch: a caller's list, or the frame mask the kernel derives the list from
struct CbgListArgs {
    const int32_t* list;               // list mode: ascending flat output pixels ...
    const int32_t* countDev;           // ... and their number on the device (null: nHost)
    int nHost;
    unsigned long long* frameMasks;    // mask mode: [2][maskWords] masks, {parity, done}, mask copy
    long maskWords;
    int wpr;
};
// ... from an entry point's arguments; maskModeOk: what the entry point asks of its other arguments in mask mode.
// CB_OK with numChanges == 0 in list mode: nothing to launch (cbg_nothing_listed).
inline int cbg_list_args(CbgListArgs& a, const int32_t* changeList, int numChanges, const int32_t* countDev,
                         uint64_t* frameMasks, bool maskModeOk, int Ho, int Wo) {
    if (frameMasks) {
        CB_REQUIRE(maskModeOk && !changeList);
        a.frameMasks = (unsigned long long*)frameMasks;
        a.maskWords = cbinfer_mask_words(Ho, Wo);
        a.wpr = cbinfer_mask_words_per_row(Wo);
    } else {
        CB_REQUIRE(changeList && numChanges >= 0 && numChanges <= Ho * Wo);
        a.list = changeList, a.countDev = countDev, a.nHost = numChanges;
    }
    return CB_OK;
}
inline bool cbg_nothing_listed(const CbgListArgs& a) { return !a.frameMasks && a.nHost == 0; }
// list mode: the number of entries the kernel reads
// (a macro: as a function, its arguments by reference or by value, cbt_conv_kernel schedules differently)
#define CBG_LIST_COUNT(L, HWo) max(0, min((L).countDev ? min(*(L).countDev, (L).nHost) : (L).nHost, HWo))

// state protocol of a frame entry point: element type of the tensors, the map the gather reads, and the detection's
// update mode -- 1: the changed pixels only (feedback);  2: wherever the values differ (the state is a copy of the input)
struct CbgFrameMode {
    int edt;
    const void* src;
    bool copyAll;
    int update;
};
inline CbgFrameMode cbg_frame_mode(const void* input, const void* prevInput, int feedbackLoop, int copyInput, int dtype) {
    CbgFrameMode m;
    m.edt = dtype == CB_F32S ? CB_F32 : dtype;
    m.src = (feedbackLoop || copyInput) ? prevInput : input;
    m.copyAll = !feedbackLoop && copyInput && prevInput != input;
    m.update = feedbackLoop ? 1 : (m.copyAll ? 2 : 0);
    return m;
}

// f(CbgArith<T, ARITH>()) for the arithmetic `dtype` (CB_F16, CB_F32S, else CB_F32: the entry points have checked it)
template <typename T_, int ARITH_>
struct CbgArith {
    typedef T_ T;
    static constexpr int ARITH = ARITH_;
};
template <typename F>
inline void cbg_dispatch_arith(int dtype, F f) {
    if (dtype == CB_F16)
        f(CbgArith<cb_half, CB_F16>());
    else if (dtype == CB_F32S)
        f(CbgArith<float, CB_F32S>());
    else
        f(CbgArith<float, CB_F32>());
}

// One launch of a detection kernel (its f32 and f16 instances): one workgroup per 64-pixel row segment of the INPUT
// map, 1 to 16 waves over the channels; the mask geometry is the OUTPUT map's.
template <typename K32, typename K16, typename Geom>
inline int cbg_launch_detect(K32 k32, K16 k16, const void* input, void* state, uint64_t* frameMasks, int C, int Hi, int Wi,
                             int Ho, int Wo, const Geom& geom, float threshold, int update, int dtype, hipStream_t s) {
    const int wprO = cbinfer_mask_words_per_row(Wo);
    const long words = cbinfer_mask_words(Ho, Wo);
    dim3 grid(cb_div_up(Wi, 64), Hi), block(64 * (C >= 32 ? 16 : C >= 8 ? 8 : C >= 4 ? 4 : C));
    auto go = [&](auto kernel, auto t) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(kernel, grid, block, 0, s, (const T*)input, (T*)state, (unsigned long long*)frameMasks, words,
                           C, Hi, Wi, Ho, Wo, wprO, geom, threshold, update);
    };
    if (dtype == CB_F16)
        go(k16, cb_half());
    else
        go(k32, float());
    return cb_launch_status();
}

// ---------------------------------------------------------------------------------------------
// detection: the channel scan of one 64-pixel row segment (pixel p of HW per plane on this lane, `valid` inside the
// row).  Wave g of the workgroup's G scans channels g, g+G, ..., two at a time; the ballots are OR-reduced through LDS
// as in cb_detect_kernel.  Returns the segment's change word, the same on every thread, and refreshes the state:
//   update 1: in[:, p] -> state[:, p] at the changed pixels only (feedback);  2: wherever the values differ at all.
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ unsigned long long cbg_detect_scan(const T* __restrict__ in, T* state, int C, long HW, long p,
                                                              bool valid, float thf, int update) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, G = blockDim.x >> 6;
    const T th = cb_threshold(thf, (T*)nullptr);
    bool chg = false;
    if (valid) {
        int c = wv;
#pragma unroll 1
        for (; c + G < C; c += 2 * G) {
            const T s0 = state[(long)c * HW + p], x0 = in[(long)c * HW + p];
            const T s1 = state[(long)(c + G) * HW + p], x1 = in[(long)(c + G) * HW + p];
            chg |= cb_changed(s0, x0, th) | cb_changed(s1, x1, th);
            if (update == 2) {
                if (cb_differs(s0, x0)) state[(long)c * HW + p] = x0;
                if (cb_differs(s1, x1)) state[(long)(c + G) * HW + p] = x1;
            }
        }
        if (c < C) {
            const T s0 = state[(long)c * HW + p], x0 = in[(long)c * HW + p];
            chg |= cb_changed(s0, x0, th);
            if (update == 2 && cb_differs(s0, x0)) state[(long)c * HW + p] = x0;
        }
    }
    __shared__ unsigned long long sm[16];
    const unsigned long long b = __ballot(chg);
    if (lane == 0) sm[wv] = b;
    __syncthreads();
    unsigned long long m = 0;
    for (int i = 0; i < G; ++i) m |= sm[i];
    if (update == 1 && ((m >> lane) & 1ull))
        for (int c = wv; c < C; c += G) state[(long)c * HW + p] = in[(long)c * HW + p];
    return m;
}

// ---------------------------------------------------------------------------------------------
// Entry k of a k -> tap table (off[CkkP], then dydx[CkkP], behind the prepared weights): tap (dy, dx) of channel c
// relative to an output pixel's BASE input pixel --
//   off[k]  = byte offset of the tap from the base pixel (64-bit arithmetic; a tap inside the map fits an int, the
//             others are never used for an address)
//   dydx[k] = (dx << 16) | (dy & 0xffff), for the border test against Hi, Wi
// tail: k is padding and gets dy = dx = -32768, outside every map the entry points admit (either one alone is not -- a
// base pixel at row 32768 or beyond brings the tap back inside a map that tall; both at once would need 2^30 pixels).
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void cbg_tab_entry(int* tab, int CkkP, int k, bool tail, int c, int dy, int dx, int Hi, int Wi) {
    tab[k] = tail ? 0 : (int)(((long)c * Hi * Wi + (long)dy * Wi + dx) * (long)sizeof(T));
    tab[CkkP + k] = tail ? (int)0x80008000u : (int)(((unsigned)dx << 16) | ((unsigned)dy & 0xffffu));
}

// ---------------------------------------------------------------------------------------------
// The change list of a mask-mode launch (cbg_conv_kernel, cbgr_conv_kernel; 256 threads): every workgroup counts the
// bits of the mask the parity selects -- thread t the words [t chunk, (t + 1) chunk), chunk = ceil(words / 256) -- and
// scans the 256 counts into sPre[257]; for its share of the words (w % gridDim.x == blockIdx.x) it writes the ascending
// list entries, the mask copy and the zeros of the OTHER mask (the next frame's); the last workgroup to arrive flips the
// parity.  Returns the number of listed pixels, `cur` the frame's mask.  sWave: four ints of LDS.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int cbg_list_from_mask(unsigned long long* frameMasks, long words, int chunk, int wpr, int Wo,
                                                  int32_t* listOut, int32_t* countOut, int* sPre, int* sWave,
                                                  const unsigned long long*& cur) {
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int G = gridDim.x;
    int* ctl = (int*)(frameMasks + 2 * words);
    const int par = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cur = frameMasks + (par ? words : 0);
    unsigned long long* other = frameMasks + (par ? 0 : words);
    unsigned long long* copy = frameMasks + 2 * words + 2;
    const long w0 = (long)t * chunk, w1 = min(words, w0 + chunk);
    int cnt = 0;
    for (long w = w0; w < w1; ++w) cnt += __popcll(cur[w]);
    // inclusive scan of the 256 chunk counts: within each wave by lane shifts, then the four wave totals
    int inc = cnt;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const int up = __shfl_up(inc, dlt, 64);
        if (lane >= dlt) inc += up;
    }
    if (lane == 63) sWave[wave] = inc;
    __syncthreads();
    for (int i = 0; i < wave; ++i) inc += sWave[i];
    sPre[t + 1] = inc;
    if (t == 0) sPre[0] = 0;
    __syncthreads();
    const int N = sPre[256];
    // every workgroup writes the list entries, the mask copy and the zeros of the OTHER mask (the next frame's) for
    // its share of the words
    int run = sPre[t];
    for (long w = w0; w < w1; ++w) {
        const unsigned long long mw = cur[w];
        if ((int)(w % G) == (int)blockIdx.x) {
            const int yy = (int)(w / wpr), xx = (int)(w % wpr) * 64;
            unsigned long long r = mw;
            int at = run;
            while (r) {
                listOut[at++] = yy * Wo + xx + __builtin_ctzll(r);
                r &= r - 1;
            }
            copy[w] = mw;
            other[w] = 0ull;
        }
        run += __popcll(mw);
    }
    if (blockIdx.x == 0 && t == 0) countOut[0] = N;
    // every workgroup has read the parity and the mask by now
    cb_flip_parity_last(ctl, par, G);
    return N;
}

// Entry q of the list (q < N checked by the caller's tile): from the mask `cur` through the scan sPre -- the last thread
// chunk whose prefix is <= q, then the words of that chunk -- or from a caller's list; -1 for an entry outside the map
// (a foreign list is not trusted with addresses).
__device__ __forceinline__ int cbg_list_entry(int q, const unsigned long long* cur, const int* sPre, long words, int chunk,
                                              int wpr, int Wo, const int32_t* list, int HWo) {
    int pix = -1;
    if (cur) {
        int lo = 0, hi = 255;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (sPre[mid] <= q) lo = mid; else hi = mid - 1;
        }
        int r = q - sPre[lo];
        long w = (long)lo * chunk;
        const long wEnd = min(words, w + chunk);
        unsigned long long mw = 0ull;
        for (; w < wEnd; ++w) {
            mw = cur[w];
            const int c = __popcll(mw);
            if (r < c) break;
            r -= c;
        }
        if (w < wEnd) pix = (int)(w / wpr) * Wo + (int)(w % wpr) * 64 + cb_select_bit(mw, r);
    } else {
        pix = list[q];
    }
    if (pix < 0 || pix >= HWo) pix = -1;
    return pix;
}

// ---------------------------------------------------------------------------------------------
// One stage's operands in registers: 8 consecutive k of a weight row (16 / 32 bytes), and 8 consecutive k of listed
// pixel pix (-1: none) gathered through the table into rb[8] -- tab: the stage's first k of this wave, uniform, so the
// taps come by scalar loads; (iy0, ix0) the pixel's base input pixel, pbase its address, zero outside the Hi x Wi map.
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void cbg_load_wrow(T (&ra)[8], const T* wsrc) {
    if constexpr (sizeof(T) == 2) {
        const uint4 v = *(const uint4*)wsrc;
        __builtin_memcpy(ra, &v, 16);
    } else {
        const float4 v0 = *(const float4*)wsrc, v1 = *(const float4*)(wsrc + 4);
        __builtin_memcpy(ra, &v0, 16);
        __builtin_memcpy(ra + 4, &v1, 16);
    }
}
// (a macro: as a function -- arguments by value or by reference, the table as base + k -- all kernels that use it
// schedule differently, profiles/gather_shared_parts.md)
#define CBG_GATHER8(T, rb, tab, CkkP, pbase, pix, iy0, ix0, Hi, Wi)                                                        \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                                       \
        const int off = (tab)[i], dd = (tab)[(CkkP) + i];                                                                 \
        const int dy = (short)(dd & 0xffff), dx = dd >> 16;                                                               \
        const bool inb = (pix) >= 0 && (unsigned)((iy0) + dy) < (unsigned)(Hi) && (unsigned)((ix0) + dx) < (unsigned)(Wi); \
        (rb)[i] = inb ? *(const T*)((pbase) + off) : T(0);                                                                \
    }

// LDS image of one operand (64 rows x 32 k) per arithmetic, and how 8 consecutive k of a row get there
template <int ARITH>
struct CbgStage;
template <>
struct CbgStage<CB_F16> {
    cb_half v[64][CBG_ROW16];
    __device__ __forceinline__ void put(int row, int k0, const cb_half (&x)[8]) {
        halfx8 t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = x[i];
        *(halfx8*)&v[row][k0] = t;
    }
};
template <>
struct CbgStage<CB_F32S> {
    unsigned short v[3][64][CBG_ROW16];
    __device__ __forceinline__ void put(int row, int k0, const float (&x)[8]) {
        ushortx8 h, m, l;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            unsigned a, b, c;
            cb_split3(x[i], a, b, c);
            h[i] = (unsigned short)a, m[i] = (unsigned short)b, l[i] = (unsigned short)c;
        }
        *(ushortx8*)&v[0][row][k0] = h;
        *(ushortx8*)&v[1][row][k0] = m;
        *(ushortx8*)&v[2][row][k0] = l;
    }
};
template <>
struct CbgStage<CB_F32> {
    float v[64][CBG_ROW32];
    __device__ __forceinline__ void put(int row, int k0, const float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[row][k0 + i] = x[i];
    }
};

template <int ARITH>
__device__ __forceinline__ floatx16 cbg_mfma_stage(const CbgStage<ARITH>& A, const CbgStage<ARITH>& B, int ra, int rb,
                                                   int lane, floatx16 acc) {
    const int kg = lane >> 5;
    if constexpr (ARITH == CB_F16) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const halfx8 a = *(const halfx8*)&A.v[ra][s * 16 + kg * 8], b = *(const halfx8*)&B.v[rb][s * 16 + kg * 8];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
    } else if constexpr (ARITH == CB_F32S) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k0 = s * 16 + kg * 8;
            const bf16x8 ah = *(const bf16x8*)&A.v[0][ra][k0], am = *(const bf16x8*)&A.v[1][ra][k0],
                         al = *(const bf16x8*)&A.v[2][ra][k0];
            const bf16x8 bh = *(const bf16x8*)&B.v[0][rb][k0], bm = *(const bf16x8*)&B.v[1][rb][k0],
                         bl = *(const bf16x8*)&B.v[2][rb][k0];
            // the six cross products above 2^-24 of the product, smallest first
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A.v[ra][2 * s + kg], B.v[rb][2 * s + kg], acc, 0, 0, 0);
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------
// The 64 x 64 x 32 tile (cbg_conv_kernel, cbt_conv_kernel).  T: element type of the tensors; ARITH: CB_F16 (T = half),
// CB_F32S or CB_F32 (T = float).  256 threads = 2 x 2 waves, one 32 x 32 MFMA tile each (output channel in the
// accumulator registers, listed pixel on the lane: a store instruction of the epilogue writes 32 pixels of one output
// plane).  Per stage of 32 k every thread loads 8 consecutive k of one weight row and gathers 8 consecutive k of one
// pixel.  The tile's three parts are statement macros over the kernel's own variables: as functions, in every form
// tried, they change the schedule and the register count of all six kernels (profiles/gather_shared_parts.md).  They
// expect in scope: T, ARITH, the LDS images sA[2], sB[2], and the thread's place in the tile
//   t, lane, wave;  gn = t & 63, gk = wave * 8 (gather: pixel row, first k of the stage);  am = t >> 2, ak = (t & 3) * 8
//   (weights: channel row, first k of the stage);  wm = wave & 1, wn = wave >> 1 (this wave's 32 x 32 tile).
//
// CBG_TILE_STAGES declares the accumulator `acc` and runs stages [s0, s1) into it.  wrow: this thread's weight row at
// its first k of stage 0; tabBase: the k -> tap table (CkkP entries per half); pix, (iy0, ix0), pbase: this thread's
// listed pixel (CBG_GATHER8).  Two LDS buffers, one barrier per stage: the loads of stage s+1 fly during the MFMAs of
// stage s and land in the other buffer behind them (whose last readers passed the previous barrier).
// ---------------------------------------------------------------------------------------------
#define CBG_TILE_STAGES(acc, wrow, tabBase, CkkP, pbase, pix, iy0, ix0, Hi, Wi, s0, s1)                                    \
    T ra[8], rb[8];                                                                                                       \
    auto load = [&](int s) {                                                                                              \
        cbg_load_wrow(ra, (wrow) + (long)s * CBG_BK);                                                                     \
        const int* tab = (tabBase) + s * CBG_BK + gk;                                                                     \
        CBG_GATHER8(T, rb, tab, CkkP, pbase, pix, iy0, ix0, Hi, Wi)                                                       \
    };                                                                                                                    \
    floatx16 acc;                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < 16; ++i) acc[i] = 0.f;                                                          \
    if ((s0) < (s1)) {                                                                                                    \
        load(s0);                                                                                                         \
        sA[0].put(am, ak, ra);                                                                                            \
        sB[0].put(gn, gk, rb);                                                                                            \
    }                                                                                                                     \
    __syncthreads();                                                                                                      \
    for (int s = (s0); s < (s1); ++s) {                                                                                   \
        const int cb = (s - (s0)) & 1;                                                                                    \
        if (s + 1 < (s1)) load(s + 1);                                                                                    \
        acc = cbg_mfma_stage<ARITH>(sA[cb], sB[cb], wm * 32 + (lane & 31), wn * 32 + (lane & 31), lane, acc);             \
        if (s + 1 < (s1)) {                                                                                               \
            sA[cb ^ 1].put(am, ak, ra);                                                                                   \
            sB[cb ^ 1].put(gn, gk, rb);                                                                                   \
        }                                                                                                                 \
        __syncthreads();                                                                                                  \
    }

// Split-k hand-off of item `item` = slice `slice` of SK > 1 (one item and one slab per workgroup): the partial tile goes
// to the workspace, and the last workgroup of the tile to arrive at `ticket` sums the SK slabs in slice order into acc;
// every other workgroup executes NOT_REDUCER (the kernels': continue).  sLast: an int of LDS.  The hand-off needs no
// agent-scope release (an L2 write-back per workgroup, which serialises the launch): every slab store is write-through
// (sc1: an agent-scope relaxed atomic store) and drained before the workgroup's ticket, every slab load is an sc1 load
// behind the reducer's acquire (MI355X_MICROARCH.md, "Inter-workgroup visibility").
// (slab = [4 waves][4 register quads][64 lanes] float4: 16 bytes per lane, 1 KB per wave instruction)
#define CBG_SPLITK_HANDOFF(acc, slabs, ticketAt, item, slice, SK, sLast, NOT_REDUCER)                                      \
    {                                                                                                                     \
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));                                                   \
        typedef float f32x4 __attribute__((ext_vector_type(4)));                                                          \
        const __amdgpu_buffer_rsrc_t srsrc =                                                                              \
            __builtin_amdgcn_make_buffer_rsrc((void*)(slabs), 0, CBG_GRID * CBG_SLAB * 4, 0x00020000);                    \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                                   \
            const f32x4 f = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};                                 \
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f), srsrc,                                   \
                                                   ((item) * (CBG_SLAB / 4) + (wave * 4 + q) * 64 + lane) * 16, 0,        \
                                                   16 /* sc1 */);                                                         \
        }                                                                                                                 \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                  \
        __syncthreads();                                                                                                  \
        int* ticket = (ticketAt);                                                                                         \
        if (t == 0) {                                                                                                     \
            const int old = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                \
            if (old == (SK) - 1) {                                                                                        \
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                                                        \
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                          \
                __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                                \
            }                                                                                                             \
            sLast = old == (SK) - 1;                                                                                      \
        }                                                                                                                 \
        __syncthreads();                                                                                                  \
        if (!sLast) NOT_REDUCER;                                                                                          \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) acc[j] = 0.f;                                                      \
        for (int sl = 0; sl < (SK); ++sl)                                                                                 \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                               \
                const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(                         \
                    srsrc, (((item) - (slice) + sl) * (CBG_SLAB / 4) + (wave * 4 + q) * 64 + lane) * 16, 0, 16 /* sc1 */)); \
                acc[4 * q] += f.x, acc[4 * q + 1] += f.y, acc[4 * q + 2] += f.z, acc[4 * q + 3] += f.w;                   \
            }                                                                                                             \
    }

// Bias, ReLU, scatter of channel tile tm into the output planes [K][HWo]; sList: the tile's 64 listed pixels, -1: none.
#define CBG_TILE_STORE(acc, sList, tm, biasV, outV, K, HWo, relu)                                                          \
    {                                                                                                                     \
        const int opix = sList[wn * 32 + (lane & 31)];                                                                    \
        if (opix >= 0) {                                                                                                  \
            T* out = (T*)(outV);                                                                                          \
            const T* bias = (const T*)(biasV);                                                                            \
            _Pragma("unroll") for (int j = 0; j < 16; ++j) {                                                              \
                const int m = (tm) * CBG_BM + wm * 32 + (j >> 2) * 8 + (lane >> 5) * 4 + (j & 3);                         \
                if (m < (K)) {                                                                                            \
                    float v = acc[j] + (bias ? (float)bias[m] : 0.f);                                                     \
                    if (relu) v = v <= 0.f ? 0.f : v;                                                                     \
                    out[(long)m * (HWo) + opix] = (T)v;                                                                   \
                }                                                                                                         \
            }                                                                                                             \
        }                                                                                                                 \
    }

}  // namespace
