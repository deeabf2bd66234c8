// Change-based fused local (neighbourhood) attention on gfx950: scores, softmax and the weighted sum of
// v in ONE launch, the volume of heads x T scores never leaving a wave's registers --
//   s[h, t]            = scale * sum_{c < d} q[h d + c, y, x] * k[h d + c, y + dy_i, x + dx_j]  (+ bias[h, t]),
//   p[h, .]            = softmax over the taps that take part,
//   out[h dv + c, y, x] = sum_t p[h, t] * v[h dv + c, y + dy_i, x + dx_j],
// t = i Dx + j over the window's taps (dy_i, dx_j) = (y0 + i step, x0 + j step), k the first C channels of the operand
// kv and v its remaining Cv.  The reference has no such operator; the contract and the arithmetic are in
// include/cbinfer_hip.h, which is the specification.  out[:, y, x] can differ from last frame's only if q changed at
// (y, x) or kv changed at one of the window's taps: the footprint of cb_corr.hip with a := q, b := kv, whose word, list
// launches and clearing launch cb_window.h holds.  A frame is
//   per operand in LIST form, one launch in front; for kv in LIST form, one launch behind (cb_window.h);
//   one launch, the whole-word walk of cb_maskwalk.h over the output mask.  The unit: the word's row y and 64 columns
//              are four 16-pixel GROUPS, one per wave; a group without a listed pixel multiplies nothing, a group with
//              one is computed WHOLE and only its listed pixels are stored, so a pixel's bits depend on its own
//              operands and on x mod 16 alone.  Loop order: head -> displacement row (ascending) -> column tile.
//              SCORES, transposed: S^T = K^T Q per 16-column tile of the strip of k's row y + dy -- M = 16 columns,
//                 N = the group's 16 pixels, K = the head's d channels.  The Q fragment (B operand) is loaded from
//                 global once per (group, head) and stays in registers over every row and tile; the k strip (A
//                 operand) is staged into LDS per (head, row) in chunks of 64 channels by all 256 threads with
//                 row-segment loads, zero for a column outside the map and a channel tail, and only the tiles that a
//                 group with a listed pixel reads.  f32: [channel][column], whose row length 16 (3 + NT) puts the four
//                 channels of a k-step on four different quarters of the banks; f16: [channel / 8][column][8].
//              BAND AND SOFTMAX in registers: the C/D layout leaves lane (n = lane & 15, g = lane >> 4) with the scores
//                 of columns 16 tile + 4 g + r, r < 4, of pixel n.  A score is kept where column - n = j step,
//                 0 <= j < Dx (and, border 'mask', the column lies in the map): scaled, biased; any other becomes -inf
//                 by a SELECT.  The softmax is the online form per pixel and head over the displacement rows: the row
//                 maximum over the lane's 4 NT values and the four lanes that share n (two __shfl_xor), m' = max(m,
//                 rowmax), f = expf(m - m'), l = l f + sum p, acc *= f, p = expf(s - m'); a pixel that has had no tap
//                 yet (m' = -inf) never evaluates -inf - -inf.  An out-of-map row stages nothing: under border 'zero'
//                 its scores are +0 (plus bias) and its values zero, under 'mask' it is skipped.
//              P V without a shuffle and without LDS for P: M = 16 channels of v, N = the 16 pixels, K = the strip's
//                 columns, which are only summed over -- so lane (n, g) hands its own p[16 tile + 4 g + r] to k-step r
//                 as it is, and the A operand reads v's strip at column 16 tile + 4 g + r.  The strip of v is
//                 [tile][channel][16 columns] (a tile padded by one channel row): a lane's four columns 4 g .. 4 g + 3
//                 of channel n are ONE 16-byte (f16: 8-byte) read, the 64 lanes of a read cover consecutive addresses.
//                 f16: p is rounded to f16 (p <= 1), two score tiles make one halfx8.  v is staged per (head, row) in
//                 blocks of 64 channels, the first with k's first chunk; 8 accumulator tiles cover dv <= 128.
//              END: out = acc / l, one division, one rounding to the dtype, stored from the registers, one run of 16
//                 pixels per channel plane, predicated on the group's mask bits; l == 0 stores +0.
// Every column of the strip is multiplied, the off-band ones by +0: the operands must be FINITE (the header says so).
// No host sync, memset, allocation, data atomics or inline assembly; all stores are plain vector stores.
#include <math.h>

#include <type_traits>

#include "cb_window.h"

// (scale, bias, the online softmax's l f + sum and the final division are specified operation by operation)
#pragma clang fp contract(off)

namespace {

#define CBT_CB 64           // channels of a staged chunk of k and of a staged block of v
#define CBT_MAXD 128        // d and dv
#define CBT_MAXHEADS 64
#define CBT_MAXSPAN 48      // x1 - x0: a group spans at most 4 column tiles

typedef _Float16 cbt_halfx4 __attribute__((ext_vector_type(4)));

struct cbt_geo {
    int C, Cv, H, W, heads, d, dv, T, NT, NTE;      // NTE: NT with P V's K padded to the dtype's k-step (f16: even)
    int masked, hasBias;                             // border 'mask'; a position bias [heads, T]
    unsigned inv;                                    // ceil(2^16 / step): d / step == (d inv) >> 16 for 0 <= d < 2^13
    float scale;
    cbw_window win;
};

// ---- staging.  Every function fills whole tiles whose bit is set in `need` (only those are read afterwards), column
// xs + col of the map row whose plane 0 starts at `row`, zero outside [0, W) and for a channel >= nch; an address is
// formed only inside the map and the block.

// k, f32: nk channels (nch rounded up to the k-step), dst[ch COLS + col]; consecutive threads, consecutive columns.
template <int COLS>
__device__ __forceinline__ void cbt_stage_k(float* __restrict__ dst, const float* __restrict__ row, long HW, int nch,
                                            int xs, int W, int tiles, unsigned need) {
    const int cols = tiles * 16, total = ((nch + 3) & ~3) * cols;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ch = e / cols, col = e - ch * cols;
        if (!((need >> (col >> 4)) & 1u)) continue;
        const int x = xs + col;
        dst[ch * COLS + col] = (x >= 0 && x < W && ch < nch) ? row[(long)ch * HW + x] : 0.f;
    }
}
// k, f16: groups of 8 channels up to the k-step of 32, dst[((ch / 8) COLS + col) 8 + ch % 8].
template <int COLS>
__device__ __forceinline__ void cbt_stage_k(cb_half* __restrict__ dst, const cb_half* __restrict__ row, long HW, int nch,
                                            int xs, int W, int tiles, unsigned need) {
    const int cols = tiles * 16, total = (((nch + 31) & ~31) >> 3) * cols;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int cg = e / cols, col = e - cg * cols;
        if (!((need >> (col >> 4)) & 1u)) continue;
        const int x = xs + col;
        const bool inx = x >= 0 && x < W;
        halfx8 p;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ch = cg * 8 + i;
            p[i] = (inx && ch < nch) ? row[(long)ch * HW + x] : cb_half(0);
        }
        *(halfx8*)&dst[(cg * COLS + col) * 8] = p;
    }
}
// v, f32: nct channel tiles, dst[((col / 16) (CBT_CB + 1) + ch) 16 + col % 16].
__device__ __forceinline__ void cbt_stage_v(float* __restrict__ dst, const float* __restrict__ row, long HW, int nch,
                                            int nct, int xs, int W, int tiles, unsigned need) {
    const int cols = tiles * 16, total = nct * 16 * cols;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ch = e / cols, col = e - ch * cols;
        if (!((need >> (col >> 4)) & 1u)) continue;
        const int x = xs + col;
        dst[((col >> 4) * (CBT_CB + 1) + ch) * 16 + (col & 15)] =
            (x >= 0 && x < W && ch < nch) ? row[(long)ch * HW + x] : 0.f;
    }
}
// v, f16: the same layout, a thread writes the four columns of one lane's read.
__device__ __forceinline__ void cbt_stage_v(cb_half* __restrict__ dst, const cb_half* __restrict__ row, long HW, int nch,
                                            int nct, int xs, int W, int tiles, unsigned need) {
    const int ncg = tiles * 4, total = nct * 16 * ncg;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ch = e / ncg, cg = e - ch * ncg;
        if (!((need >> (cg >> 2)) & 1u)) continue;
        cbt_halfx4 p;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = xs + cg * 4 + i;
            p[i] = (x >= 0 && x < W && ch < nch) ? row[(long)ch * HW + x] : cb_half(0);
        }
        *(cbt_halfx4*)&dst[((cg >> 2) * (CBT_CB + 1) + ch) * 16 + (cg & 3) * 4] = p;
    }
}

// q [C, H, W], kv [C + Cv, H, W], bias [heads, T] f32 or NULL, out [Cv, H, W].  maskQ / maskKV / all as cbc_corr_kernel's
// maskA / maskB / all.  NTMAX (even) >= g.NTE sizes the score registers and the LDS.
template <typename T, int NTMAX>
__global__ __launch_bounds__(256) void cbt_attend_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                        const float* __restrict__ bias, T* __restrict__ out,
                                                        const unsigned long long* __restrict__ maskQ,
                                                        const unsigned long long* __restrict__ maskKV, int all,
                                                        unsigned long long* bits,
                                                        unsigned long long* __restrict__ maskCopy, long words,
                                                        cbt_geo g, int wpr) {
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int TILES = 3 + NTMAX, COLS = 16 * TILES;
    constexpr int QCH = F16 ? 32 : 4;                 // channels of one k-step of the scores
    constexpr int QREGS = CBT_MAXD / QCH;             // the Q fragment: 32 registers (f32), 4 x 4 (f16)
    constexpr int KS = CBT_CB / QCH;                  // k-steps of a chunk of k
    using qfrag = typename std::conditional<F16, halfx8, float>::type;
    __shared__ __attribute__((aligned(16))) T sK[CBT_CB * COLS];
    __shared__ __attribute__((aligned(16))) T sV[TILES * (CBT_CB + 1) * 16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, gq = lane >> 4;
    const long HW = (long)g.H * g.W;
    const T* __restrict__ v = kv + (long)g.C * HW;
    cb_walk_word_units(
        bits, maskCopy, words, g.W, wpr, all,
        [&](long wd, int y, int tile) -> unsigned long long {
            if (all) return 0ull;
            return cbw_footprint_word(maskQ, maskKV, wd, y, tile, g.H, wpr, g.win, lane);
        },
        [&](unsigned long long word, int y, int tile) {
            const int xw = tile * 64, xg = xw + 16 * wave;
            // this wave's group, and the tiles of the strips that the groups with a listed pixel read
            const unsigned grp = __builtin_amdgcn_readfirstlane((unsigned)(word >> (16 * wave)) & 0xffffu);
            unsigned need = 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if ((word >> (16 * u)) & 0xffffull) need |= ((1u << g.NTE) - 1u) << u;
            const bool pix = xg + n < g.W;                 // (a group may be cut by the row end)
            const bool listed = (grp >> n) & 1u;           // (a set bit is a pixel of the row: cb_valid_mask)
            for (int h = 0; h < g.heads; ++h) {
                // the Q fragment: channel on lane >> 4, pixel on lane & 15; zero beyond d and beyond the row
                qfrag qf[QREGS];
                {
                    const T* qp = q + (long)h * g.d * HW + (long)y * g.W + xg + n;
#pragma unroll
                    for (int s = 0; s < QREGS; ++s) {
                        if constexpr (F16) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const int c = 32 * s + 8 * gq + e;
                                qf[s][e] = (grp != 0u && pix && c < g.d) ? qp[(long)c * HW] : cb_half(0);
                            }
                        } else {
                            const int c = 4 * s + gq;
                            qf[s] = (grp != 0u && pix && c < g.d) ? qp[(long)c * HW] : 0.f;
                        }
                    }
                }
                float m = -INFINITY, l = 0.f;      // the running maximum and sum of pixel n (the same on its 4 lanes)
                floatx4 acc[8];                    // channel 64 vb + 16 ct + 4 gq + r of pixel n
#pragma unroll
                for (int a = 0; a < 8; ++a) acc[a] = floatx4{0.f, 0.f, 0.f, 0.f};
                for (int di = 0; di < g.win.Dy; ++di) {
                    const int yy = y + g.win.y0 + di * g.win.step;
                    const bool inside = yy >= 0 && yy < g.H;      // (uniform over the workgroup)
                    if (!inside && g.masked) continue;            // (a row wholly outside takes no part)
                    floatx4 S[NTMAX];
#pragma unroll
                    for (int t = 0; t < NTMAX; ++t) S[t] = floatx4{0.f, 0.f, 0.f, 0.f};
                    if (inside) {
#pragma unroll
                        for (int cc = 0; cc < CBT_MAXD / CBT_CB; ++cc) {
                            if (cc * CBT_CB >= g.d) continue;
                            const int nch = min(CBT_CB, g.d - cc * CBT_CB);
                            __syncthreads();      // the fragments staged before have been read
                            cbt_stage_k<COLS>(sK, kv + ((long)h * g.d + cc * CBT_CB) * HW + (long)yy * g.W, HW, nch,
                                              xw + g.win.x0, g.W, 3 + g.NTE, need);
                            if (cc == 0) {
                                const int nv = min(CBT_CB, g.dv);
                                cbt_stage_v(sV, v + (long)h * g.dv * HW + (long)yy * g.W, HW, nv, (nv + 15) >> 4,
                                            xw + g.win.x0, g.W, 3 + g.NTE, need);
                            }
                            __syncthreads();
                            if (grp == 0u) continue;      // (wave-uniform; the barriers are outside it)
#pragma unroll
                            for (int s = 0; s < KS; ++s) {
                                if (s * QCH >= nch) continue;
#pragma unroll
                                for (int t = 0; t < NTMAX; ++t) {
                                    if (t >= g.NT) continue;
                                    if constexpr (F16) {
                                        const halfx8 av =
                                            *(const halfx8*)&sK[((4 * s + gq) * COLS + 16 * (wave + t) + n) * 8];
                                        S[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, qf[cc * KS + s], S[t], 0, 0, 0);
                                    } else {
                                        const float av = sK[(4 * s + gq) * COLS + 16 * (wave + t) + n];
                                        S[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, qf[cc * KS + s], S[t], 0, 0, 0);
                                    }
                                }
                            }
                        }
                    }
                    if (grp != 0u) {
                        // the band: lane (n, gq) holds columns 16 t + 4 gq + r of pixel n; -inf by a select
                        const float* brow = g.hasBias ? bias + (long)h * g.T + (long)di * g.win.Dx : nullptr;
                        float rowmax = -INFINITY;
#pragma unroll
                        for (int t = 0; t < NTMAX; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int col = 16 * t + 4 * gq + r, dd = col - n;
                                const int j = dd >= 0 ? (int)(((unsigned)dd * g.inv) >> 16) : 0;
                                bool on = t < g.NT && dd >= 0 && j * g.win.step == dd && j < g.win.Dx;
                                if (g.masked) {
                                    const int xc = xg + g.win.x0 + col;
                                    on = on && xc >= 0 && xc < g.W;
                                }
                                float s = S[t][r] * g.scale;
                                if (g.hasBias) s = s + (on ? brow[j] : 0.f);
                                s = on ? s : -INFINITY;
                                S[t][r] = s;
                                rowmax = fmaxf(rowmax, s);
                            }
                        rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 16));
                        rowmax = fmaxf(rowmax, __shfl_xor(rowmax, 32));
                        const float mn = fmaxf(m, rowmax);
                        const float ms = mn > -INFINITY ? mn : 0.f;      // (no tap yet: -inf - -inf is never formed)
                        const float f = expf(m - ms);
                        float sum = 0.f;
#pragma unroll
                        for (int t = 0; t < NTMAX; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float p = S[t][r] > -INFINITY ? expf(S[t][r] - ms) : 0.f;
                                S[t][r] = p;
                                sum = sum + p;
                            }
                        sum = sum + __shfl_xor(sum, 16);
                        sum = sum + __shfl_xor(sum, 32);
                        l = l * f + sum;
                        m = mn;
#pragma unroll
                        for (int a = 0; a < 8; ++a)
#pragma unroll
                            for (int r = 0; r < 4; ++r) acc[a][r] = acc[a][r] * f;
                    }
                    if (!inside) continue;      // (border 'zero': the row's values are zero)
#pragma unroll
                    for (int vb = 0; vb < CBT_MAXD / CBT_CB; ++vb) {
                        if (vb * CBT_CB >= g.dv) continue;
                        const int nv = min(CBT_CB, g.dv - vb * CBT_CB), nct = (nv + 15) >> 4;
                        if (vb > 0) {
                            __syncthreads();      // the block before has been read
                            cbt_stage_v(sV, v + ((long)h * g.dv + vb * CBT_CB) * HW + (long)yy * g.W, HW, nv, nct,
                                        xw + g.win.x0, g.W, 3 + g.NTE, need);
                            __syncthreads();
                        }
                        if (grp == 0u) continue;
                        if constexpr (F16) {
#pragma unroll
                            for (int u = 0; u < NTMAX / 2; ++u) {
                                if (2 * u >= g.NTE) continue;
                                halfx8 pb;      // K index 8 gq + e: tile 2 u + (e >> 2), column 4 gq + (e & 3)
#pragma unroll
                                for (int e = 0; e < 8; ++e) pb[e] = (cb_half)S[2 * u + (e >> 2)][e & 3];
#pragma unroll
                                for (int ct = 0; ct < 4; ++ct) {
                                    if (ct >= nct) continue;
                                    const T* a0 = &sV[((wave + 2 * u) * (CBT_CB + 1) + 16 * ct + n) * 16 + 4 * gq];
                                    const cbt_halfx4 lo = *(const cbt_halfx4*)a0;
                                    const cbt_halfx4 hi = *(const cbt_halfx4*)(a0 + (CBT_CB + 1) * 16);
                                    const halfx8 av = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                                    acc[4 * vb + ct] =
                                        __builtin_amdgcn_mfma_f32_16x16x32_f16(av, pb, acc[4 * vb + ct], 0, 0, 0);
                                }
                            }
                        } else {
#pragma unroll
                            for (int t = 0; t < NTMAX; ++t) {
                                if (t >= g.NT) continue;
#pragma unroll
                                for (int ct = 0; ct < 4; ++ct) {
                                    if (ct >= nct) continue;
                                    const floatx4 av = *(const floatx4*)&sV[((wave + t) * (CBT_CB + 1) +
                                                                                    16 * ct + n) * 16 + 4 * gq];
#pragma unroll
                                    for (int r = 0; r < 4; ++r)
                                        acc[4 * vb + ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                            av[r], S[t][r], acc[4 * vb + ct], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
                // C/D layout of the 16x16 MFMAs: pixel lane & 15, channel 4 (lane >> 4) + register
                if (grp != 0u && listed) {
                    T* o = out + (long)h * g.dv * HW + (long)y * g.W + xg + n;
#pragma unroll
                    for (int a = 0; a < 8; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ch = 16 * a + 4 * gq + r;
                            // one division, one rounding to the dtype; a pixel without a tap is +0
                            if (ch < g.dv) o[(long)ch * HW] = (T)(l > 0.f ? acc[a][r] / l : 0.f);
                        }
                }
            }
        });
}

template <typename T>
void cbt_launch(const void* q, const void* kv, const float* bias, void* out, const uint64_t* maskQ,
                const uint64_t* maskKV, int all, uint64_t* bits, uint64_t* maskCopy, cbt_geo g, hipStream_t s) {
    const int wpr = (g.W + 63) / 64;
    const long words = (long)g.H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
    g.NTE = sizeof(T) == 2 ? g.NT + (g.NT & 1) : g.NT;
#define CBT_GO(NTMAX)                                                                                                  \
    hipLaunchKernelGGL((cbt_attend_kernel<T, NTMAX>), grid, block, 0, s, (const T*)q, (const T*)kv, bias, (T*)out,      \
                       (const unsigned long long*)maskQ, (const unsigned long long*)maskKV, all,                       \
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, g, wpr)
    if (g.NT <= 2)
        CBT_GO(2);
    else
        CBT_GO(4);
#undef CBT_GO
}

}  // namespace

int cbinfer_attend_supported(const cbAttend* a, int C, int Cv, int H, int W) {
    if (!a || !cbw_window_ok(a->y0, a->y1, a->x0, a->x1, a->step) || a->x1 - a->x0 > CBT_MAXSPAN) return 0;
    if (!(a->heads >= 1 && a->heads <= CBT_MAXHEADS && C >= 1 && Cv >= 1 && H >= 1 && W >= 1)) return 0;
    if (C % a->heads || Cv % a->heads || C / a->heads > CBT_MAXD || Cv / a->heads > CBT_MAXD) return 0;
    if (!((a->border == CB_ATTEND_MASK || a->border == CB_ATTEND_ZERO) && (a->hasBias == 0 || a->hasBias == 1))) return 0;
    if (!(a->scale == a->scale && fabsf(a->scale) <= 3.0e38f)) return 0;      // (finite)
    // (a list addresses a pixel with an int32; C + Cv <= 2 x 64 x 128 planes is within the other operators' limit)
    return (long)H * W < (1l << 31);
}

int cbinfer_cbattend_forward(const void* q, const void* kv, const float* positionBias, void* outputState,
                             const uint64_t* maskQ, const int32_t* listQ, int capQ, const int32_t* countQ,
                             const uint64_t* maskKV, const int32_t* listKV, int capKV, const int32_t* countKV,
                             uint64_t* kvBits, uint64_t* bits, uint64_t* maskCopy, int C, int Cv, int H, int W,
                             const cbAttend* attend, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    const cbw_forms f = {maskQ, listQ, capQ, countQ, maskKV, listKV, capKV, countKV, kvBits, bits, maskCopy};
    CB_REQUIRE(q && kv && outputState && outputState != q && outputState != kv && q != kv);
    CB_REQUIRE(cbw_forms_ok(f));
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_attend_supported(attend, C, Cv, H, W));
    CB_REQUIRE((attend->hasBias != 0) == (positionBias != nullptr));
    cbt_geo g;
    g.C = C, g.Cv = Cv, g.H = H, g.W = W, g.heads = attend->heads, g.d = C / attend->heads, g.dv = Cv / attend->heads;
    g.win.y0 = attend->y0, g.win.x0 = attend->x0, g.win.step = attend->step;
    g.win.Dy = (attend->y1 - attend->y0) / attend->step + 1;
    g.win.Dx = (attend->x1 - attend->x0) / attend->step + 1;
    g.T = g.win.Dy * g.win.Dx;
    g.NT = g.NTE = (16 + attend->x1 - attend->x0 + 15) / 16;      // (at most 4)
    g.masked = attend->border == CB_ATTEND_MASK, g.hasBias = attend->hasBias;
    g.inv = (65536u + attend->step - 1) / attend->step;
    g.scale = attend->scale;
    const hipStream_t s = (hipStream_t)stream;
    cbw_frame fr;
    int st = cbw_lists_to_bits(f, H, W, stream, &fr);
    if (st != CB_OK) return st;
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbt_launch<decltype(t)>(q, kv, positionBias, outputState, fr.mA, fr.mB, fr.all, bits, maskCopy, g, s);
    });
    st = cb_launch_status();
    return (st != CB_OK || !fr.bList) ? st : cbw_clear_list(f, H, W, s);
}
