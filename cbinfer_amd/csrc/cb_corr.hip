// Change-based correlation layer (the cost volume of FlowNet / PWC-Net / DispNet-type networks) on gfx950:
//   out[i Dx + j, y, x] = scale * sum_c a[c, y, x] * b[c, y + y0 + i step, x + x0 + j step],   scale = 1/C or 1,
// a tap outside the map contributing nothing.  The reference has no such operator; the contract and the arithmetic are
// in include/cbinfer_hip.h, which is the specification.  Every producer of this library leaves the pixels outside its
// change list bit for bit as they were, so out[:, y, x] can differ from last frame's only if `a` changed at (y, x) or b
// changed at one of the window's taps: recomputing there is the dense result exactly, without a threshold.  Unlike the
// grid sampling this IS a contraction -- per displacement row a banded product of a^T with a strip of b over the
// channel axis -- and runs on the matrix unit.  A frame is
//   per operand in LIST form, one launch in front (cbw_lists_to_bits of cb_window.h): a's list into the working mask of
//              the output, b's into a working mask of its own;
//   one launch, the whole-word walk of cb_maskwalk.h (cb_walk_word_units) over the output mask.  makeWord: a's mask
//              word ORed with the windows of b's mask at every displacement -- the (i, j) shifts dealt over the 64 lanes
//              of every wave, two 64-bit loads and a funnel shift each, OR-reduced by a butterfly: every wave makes the
//              same word.  The unit: the word's row y and 64 columns are four 16-column GROUPS, one per wave; a group
//              without a listed pixel does nothing, a group with one is computed WHOLE -- 16 pixels x all Dy Dx
//              channels -- and only its listed pixels are stored.  A pixel's bits therefore depend on its own operands
//              and on x mod 16 alone.  Per displacement row the 16 pixels meet NT = ceil((16 + x1 - x0) / 16) column
//              tiles of b's row y + dy: per k-chunk (16 channels in f32, 32 in f16) the 256 threads stage the a strip
//              and the b strip into LDS as [16-column tile][k][16 columns] (f16: [tile][k / 8][column][8 k]) by
//              coalesced row-segment loads -- zeros for a column outside the map and for the channel tail, and only the
//              tiles a group with listed pixels reads --, so that an MFMA fragment read is 64 consecutive lanes on
//              consecutive addresses; v_mfma_f32_16x16x4_f32 / v_mfma_f32_16x16x32_f16 accumulate the NT tiles of the
//              row in NT x 4 registers.  The displacement rows are the OUTER loop (the budget is in DESIGN 5.33).  Of
//              the 16 x 16 NT products of a row, element (pixel i, column 16 t + j) is channel (16 t + j - i) / step
//              where that is an integer in [0, Dx): the band goes through LDS as [channel][16 pixels], is scaled,
//              rounded once and stored with the lanes along the pixel axis -- one run of 16 pixels per output plane;
//   for b in LIST form, one launch behind: zero to the words of b's working mask that the list named (the frame launch
//              reads that mask from every workgroup, so it cannot clear it itself).
// No host sync, memset, allocation, data atomics or inline assembly; all stores are plain vector stores.
#include "cb_window.h"

// (the one f32 operation outside the matrix unit is the multiply by the scale: nothing to contract, and it stays so)
#pragma clang fp contract(off)

namespace {

struct cbc_geo {
    int C, H, W, y0, x0, step, Dy, Dx, NT;
    float scale;
};

// the k-chunk of a dtype: KC channels per LDS stage, VEC of them side by side in LDS (one MFMA operand register set)
template <typename T>
struct cbc_chunk;
template <>
struct cbc_chunk<float> {
    static constexpr int KC = 16, VEC = 1;
};
template <>
struct cbc_chunk<cb_half> {
    static constexpr int KC = 32, VEC = 8;
};

// Stage KC channels from c0 of `tiles` 16-column tiles of one map row into dst: column xs + 16 ti + j of channel
// c0 + kv VEC + e goes to dst[((ti KV + kv) 16 + j) VEC + e]; zero for a column outside [0, W) or a channel >= C.  Only
// tiles whose bit is set in `need` are written (and only those are read afterwards).  row: the row's first pixel in
// channel plane 0.  Consecutive threads take consecutive columns of one channel (group): coalesced row segments.
template <typename T>
__device__ __forceinline__ void cbc_stage(T* __restrict__ dst, const T* __restrict__ row, long HW, int c0, int C, int xs,
                                          int W, int tiles, unsigned need) {
    constexpr int VEC = cbc_chunk<T>::VEC, KV = cbc_chunk<T>::KC / VEC;
    const int cols = tiles * 16, total = cols * KV;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int kv = e / cols, col = e - kv * cols, ti = col >> 4;
        if (!((need >> ti) & 1u)) continue;
        const int x = xs + col;
        const bool inx = x >= 0 && x < W;
        T v[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int c = c0 + kv * VEC + i;
            v[i] = (inx && c < C) ? row[(long)c * HW + x] : T(0);      // (an address is formed only inside the map)
        }
        T* d = dst + ((ti * KV + kv) * 16 + (col & 15)) * VEC;
        if constexpr (VEC == 8) {
            halfx8 p;
#pragma unroll
            for (int i = 0; i < 8; ++i) p[i] = v[i];
            *(halfx8*)d = p;
        } else {
            d[0] = v[0];
        }
    }
}

// a, b [C, H, W], out [Dy Dx, H, W].  maskA: a's change mask of this frame, or NULL (a list is in `bits` already);
// maskB: b's -- its own, or the working mask its list went into --, or NULL: b did not change; all: every pixel is
// listed, neither mask is read.  NTMAX >= g.NT sizes the accumulators and the LDS.
template <typename T, int NTMAX>
__global__ __launch_bounds__(256) void cbc_corr_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                      T* __restrict__ out,
                                                      const unsigned long long* __restrict__ maskA,
                                                      const unsigned long long* __restrict__ maskB, int all,
                                                      unsigned long long* bits,
                                                      unsigned long long* __restrict__ maskCopy, long words, cbc_geo g,
                                                      int wpr) {
    constexpr int KC = cbc_chunk<T>::KC, TILE = KC * 16;      // elements of one staged 16-column tile
    constexpr int DXMAX = 16 * NTMAX - 15;                      // (Dx <= x1 - x0 + 1 <= 16 NT - 15)
    __shared__ __attribute__((aligned(16))) T sA[4 * TILE];
    __shared__ __attribute__((aligned(16))) T sB[(3 + NTMAX) * TILE];
    __shared__ float sBand[4][DXMAX][17];      // per wave [channel][pixel], a row padded by one bank
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long HW = (long)g.H * g.W;
    const cbw_window win = {g.y0, g.x0, g.step, g.Dy, g.Dx};
    cb_walk_word_units(
        bits, maskCopy, words, g.W, wpr, all,
        [&](long w, int y, int tile) -> unsigned long long {
            if (all) return 0ull;
            return cbw_footprint_word(maskA, maskB, w, y, tile, g.H, wpr, win, lane);
        },
        [&](unsigned long long word, int y, int tile) {
            const int xw = tile * 64;
            // this wave's group, and the tiles that the groups with a listed pixel read
            const unsigned grp = __builtin_amdgcn_readfirstlane((unsigned)(word >> (16 * wave)) & 0xffffu);
            unsigned needA = 0u, needB = 0u;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if ((word >> (16 * v)) & 0xffffull) {
                    needA |= 1u << v;
                    needB |= ((1u << g.NT) - 1u) << v;
                }
            for (int di = 0; di < g.Dy; ++di) {
                const int yy = y + g.y0 + di * g.step;
                const bool inside = yy >= 0 && yy < g.H;      // (a row wholly outside the map: no MFMA, zeros)
                floatx4 acc[NTMAX];
#pragma unroll
                for (int t = 0; t < NTMAX; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
                if (inside) {
                    for (int c0 = 0; c0 < g.C; c0 += KC) {
                        __syncthreads();      // the fragments of the chunk before have been read
                        cbc_stage<T>(sA, a + (long)y * g.W, HW, c0, g.C, xw, g.W, 4, needA);
                        cbc_stage<T>(sB, b + (long)yy * g.W, HW, c0, g.C, xw + g.x0, g.W, 3 + g.NT, needB);
                        __syncthreads();
                        if (grp == 0u) continue;      // (wave-uniform; the barriers above are outside it)
                        if constexpr (cbc_chunk<T>::VEC == 8) {
                            const halfx8 av = *(const halfx8*)&sA[wave * TILE + lane * 8];
#pragma unroll
                            for (int t = 0; t < NTMAX; ++t)
                                if (t < g.NT) {
                                    const halfx8 bv = *(const halfx8*)&sB[(wave + t) * TILE + lane * 8];
                                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc[t], 0, 0, 0);
                                }
                        } else {
#pragma unroll
                            for (int s = 0; s < KC / 4; ++s) {
                                const float av = sA[wave * TILE + s * 64 + lane];
#pragma unroll
                                for (int t = 0; t < NTMAX; ++t)
                                    if (t < g.NT) {
                                        const float bv = sB[(wave + t) * TILE + s * 64 + lane];
                                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
                                    }
                            }
                        }
                    }
                    // the band: C/D layout of the 16x16 MFMAs -- column lane & 15, row (pixel) 4 (lane >> 4) + register
                    if (grp != 0u) {
#pragma unroll
                        for (int t = 0; t < NTMAX; ++t)
                            if (t < g.NT) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int i = 4 * (lane >> 4) + r, d = 16 * t + (lane & 15) - i;
                                    const int q = d / g.step;
                                    if (d >= 0 && q * g.step == d && q < g.Dx) sBand[wave][q][i] = acc[t][r];
                                }
                            }
                    }
                    __syncthreads();
                }
                if (grp != 0u) {
                    const int i = lane & 15;
                    const bool listed = (grp >> i) & 1u;      // (a set bit is a pixel of the row: cb_valid_mask)
                    T* o = out + (long)di * g.Dx * HW + (long)y * g.W + xw + 16 * wave + i;
                    for (int q = lane >> 4; q < g.Dx; q += 4) {
                        const float v = inside ? sBand[wave][q][i] : 0.f;
                        if (listed) o[(long)q * HW] = (T)(v * g.scale);      // one multiply, one rounding to the dtype
                    }
                }
            }
            __syncthreads();      // every wave has read its band before the next word's is written
        });
}

template <typename T>
void cbc_launch(const void* a, const void* b, void* out, const uint64_t* maskA, const uint64_t* maskB, int all,
                uint64_t* bits, uint64_t* maskCopy, const cbc_geo& g, hipStream_t s) {
    const int wpr = (g.W + 63) / 64;
    const long words = (long)g.H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBC_GO(NTMAX)                                                                                                  \
    hipLaunchKernelGGL((cbc_corr_kernel<T, NTMAX>), grid, block, 0, s, (const T*)a, (const T*)b, (T*)out,               \
                       (const unsigned long long*)maskA, (const unsigned long long*)maskB, all,                        \
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, g, wpr)
    if (g.NT <= 2)
        CBC_GO(2);
    else if (g.NT <= 4)
        CBC_GO(4);
    else
        CBC_GO(9);
#undef CBC_GO
}

}  // namespace

int cbinfer_correlation_supported(const cbCorr* c, int C, int H, int W) {
    if (!c) return 0;
    if (!(cbw_window_ok(c->y0, c->y1, c->x0, c->x1, c->step) && (c->normalize == 0 || c->normalize == 1))) return 0;
    // (a list addresses a pixel with an int32; C is within the other operators' limit)
    return C >= 1 && H >= 1 && W >= 1 && (long)H * W < (1l << 31) && (long)C * 64 < (1l << 31);
}

int cbinfer_cbcorrelation_forward(const void* a, const void* b, void* outputState, const uint64_t* maskA,
                                  const int32_t* listA, int capA, const int32_t* countA, const uint64_t* maskB,
                                  const int32_t* listB, int capB, const int32_t* countB, uint64_t* bBits, uint64_t* bits,
                                  uint64_t* maskCopy, int C, int H, int W, const cbCorr* corr, int dtype,
                                  cbStream_t stream) {
    // (every argument is checked before the first launch)
    const cbw_forms f = {maskA, listA, capA, countA, maskB, listB, capB, countB, bBits, bits, maskCopy};
    CB_REQUIRE(a && b && outputState && outputState != a && outputState != b);
    CB_REQUIRE(cbw_forms_ok(f));
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_correlation_supported(corr, C, H, W));
    cbc_geo g;
    g.C = C, g.H = H, g.W = W, g.y0 = corr->y0, g.x0 = corr->x0, g.step = corr->step;
    g.Dy = (corr->y1 - corr->y0) / corr->step + 1;
    g.Dx = (corr->x1 - corr->x0) / corr->step + 1;
    g.NT = (16 + corr->x1 - corr->x0 + 15) / 16;      // (at most 9)
    g.scale = corr->normalize ? 1.f / (float)C : 1.f;
    const hipStream_t s = (hipStream_t)stream;
    cbw_frame fr;
    int st = cbw_lists_to_bits(f, H, W, stream, &fr);
    if (st != CB_OK) return st;
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbc_launch<decltype(t)>(a, b, outputState, fr.mA, fr.mB, fr.all, bits, maskCopy, g, s);
    });
    st = cb_launch_status();
    return (st != CB_OK || !fr.bList) ? st : cbw_clear_list(f, H, W, s);
}
