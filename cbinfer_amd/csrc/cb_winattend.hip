// Change-based partitioned window attention on gfx950 (Swin-type blocks): the map is cut into
// non-overlapping Wy x Wx CELLS on a grid shifted by (sy, sx), clipped at the map's edge; every token of a cell attends
// to every token of the same cell --
//   s[i, j]            = scale * sum_{c < d} q[h d + c, i] * k[h d + c, j]  (+ bias[h, yi - yj + Wy - 1, xi - xj + Wx - 1]),
//   p[i, .]            = softmax over the cell's N tokens,
//   out[h dv + c, i]   = sum_j p[i, j] * v[h dv + c, j],
// i, j the cell's in-map pixels row-major, k the first C channels of the operand kv and v its remaining Cv.  The
// reference has no such operator; the contract and the arithmetic are in include/cbinfer_hip.h, which is the
// specification.  out at a pixel can differ from last frame's only if q changed there or kv changed anywhere in the
// pixel's cell.  A frame is
//   per operand in LIST form, one launch in front (cb_window.h: q's list into `bits`, kv's into `kvBits`);
//   one FOOTPRINT launch, the whole-word walk of cb_maskwalk.h: a word of the frame's mask is q's word ORed with the
//              column segments of the cells that lie over it and hold a set bit of kv's mask; it goes to maskCopy,
//              `bits` is zeroed;
//   one FRAME launch, grid units (cell, head), four waves each.  A unit reads its cell's segments of maskCopy -- lane r
//              the row r -- and ends there if none has a bit (an IDLE unit).  Otherwise the cell is computed WHOLE and
//              only its listed pixels are stored, so a pixel's bits depend on its cell's operands alone.  Head 0's unit
//              zeroes the cell's words of `kvBits` behind a list of kv (no unit reads them): no launch behind the frame.
//              STAGING, once per unit: k (N x d) and v (N x dv) of the cell into LDS, zero for the token tail of a
//                 16-token tile, for the channel tail of a k-step (k) or a 16-channel tile (v).  A wave instruction
//                 covers 64 / 32 / 16 consecutive tokens -- several cell rows -- of 1 / 2 / 4 channels.  k, f32:
//                 [channel][token] with a row of 80 or 144 tokens (= 16 mod 64: the four channels of a k-step lie on
//                 four different quarters of the banks); f16: [channel / 8][token][8].  v: [tile][channel][16 tokens]:
//                 a lane's four tokens 4 g .. 4 g + 3 of channel n are ONE 16-byte (f16: 8-byte) read, the 64 lanes of
//                 a read cover consecutive addresses.  The head's bias table and the tokens' (row, column) codes go to
//                 LDS as well.
//              SCORES, transposed: S^T = K^T Q, M = a tile of 16 keys, N = 16 queries, K = the head's d channels.
//                 Waves take the cell's query tiles round-robin; the Q fragment (B operand) is loaded from global once
//                 per query tile.  The C/D layout leaves lane (n = lane & 15, g = lane >> 4) with the scores of keys
//                 16 t + 4 g + r, r < 4, of query n: all N scores of a query are 4 NT <= 36 registers over four lanes.
//              SOFTMAX, plain two-pass in registers: scaled, biased, a padding key -inf by a SELECT; the maximum over
//                 the lane's values and the four lanes of a query (two __shfl_xor); p = expf(s - m); the sum per lane
//                 over its keys ascending, then over the four lanes pairwise.  A cell holds the query itself: l >= 1.
//              P V without a shuffle and without LDS for P: M = 16 channels of v, N = the 16 queries, K = keys, which
//                 are only summed over -- lane (n, g) hands its own p[16 t + 4 g + r] to k-step r as it is.  f16: p is
//                 rounded to f16 (p <= 1), two key tiles make one halfx8 (an odd tile count is padded with a zero tile).
//              END: out = acc / l, one division, one rounding to the dtype, stored from the registers.
// Launches per frame: mask / bare operands 2, one more per operand in list form (the sliding mode: 1, one more per list
// and one behind a list of kv).  The padding tokens are multiplied as +0: the operands must be FINITE.
// No host sync, memset, allocation, data atomics or inline assembly; all stores are plain vector stores.
#include <math.h>

#include <type_traits>

#include "cb_window.h"

// (scale, bias, the softmax's sum and the final division are specified operation by operation)
#pragma clang fp contract(off)

namespace {

#define CBN_MAXW 16         // Wy, Wx
#define CBN_MAXN 144        // tokens of a cell: nine 16-token tiles
#define CBN_MAXD 64         // d and dv
#define CBN_MAXHEADS 64
#define CBN_MAXBIAS ((2 * CBN_MAXW - 1) * (2 * CBN_MAXW - 1))

typedef _Float16 cbn_halfx4 __attribute__((ext_vector_type(4)));

struct cbn_geo {
    int C, Cv, H, W, heads, d, dv, Wy, Wx;
    int oy, ox;             // the grid's origin, <= 0: cell (cy, cx) is rows oy + cy Wy .., columns ox + cx Wx .., clipped
    int ncy, ncx, hasBias;
    float scale;
};

// bits lo .. hi - 1 of a mask word, cut to the word
__device__ __forceinline__ unsigned long long cbn_range(int lo, int hi) {
    lo = max(lo, 0), hi = min(hi, 64);
    if (lo >= hi) return 0ull;
    const unsigned long long upto = hi == 64 ? ~0ull : (1ull << hi) - 1ull;
    return upto & ~((1ull << lo) - 1ull);
}

// The footprint launch.  maskQ: q's change mask or NULL (a list is in `bits` already); maskKV: kv's -- its own, or the
// working mask its list went into --, or NULL: kv did not change; all: every pixel is listed, neither mask is read.
__global__ __launch_bounds__(256) void cbn_footprint_kernel(const unsigned long long* __restrict__ maskQ,
                                                           const unsigned long long* __restrict__ maskKV, int all,
                                                           unsigned long long* bits,
                                                           unsigned long long* __restrict__ maskCopy, long words,
                                                           cbn_geo g, int wpr) {
    const int lane = threadIdx.x & 63;
    cb_walk_word_units(
        bits, maskCopy, words, g.W, wpr, all,
        [&](long wd, int y, int tile) -> unsigned long long {      // (every wave makes the same word)
            if (all) return 0ull;
            unsigned long long word = maskQ ? maskQ[wd] : 0ull;
            if (!maskKV) return word;
            const int cy = (y - g.oy) / g.Wy;
            const int r0 = max(0, g.oy + cy * g.Wy), r1 = min(g.H, g.oy + (cy + 1) * g.Wy);
            // kv's mask ORed over the rows of the cell row, words tile - 1 .. tile + 1: lane = (row, word)
            const int r = lane >> 2, t = lane & 3, wi = tile - 1 + t;
            unsigned long long m = (t < 3 && r0 + r < r1 && wi >= 0 && wi < wpr) ? maskKV[(long)(r0 + r) * wpr + wi] : 0ull;
#pragma unroll
            for (int o = 4; o <= 32; o <<= 1) m |= __shfl_xor(m, o);
            const unsigned long long prev = __shfl(m, 0), own = __shfl(m, 1), next = __shfl(m, 2);
            // the cells over this word's columns, one per lane: a cell that holds a bit lists its whole segment
            const int x0 = tile * 64, cx0 = (x0 - g.ox) / g.Wx, cx1 = (min(x0 + 63, g.W - 1) - g.ox) / g.Wx;
            unsigned long long f = 0ull;
            for (int cx = cx0 + lane; cx <= cx1; cx += 64) {
                const int xa = max(0, g.ox + cx * g.Wx) - x0, xb = min(g.W, g.ox + (cx + 1) * g.Wx) - x0;
                const unsigned long long hit = (prev & cbn_range(xa + 64, xb + 64)) | (own & cbn_range(xa, xb)) |
                                               (next & cbn_range(xa - 64, xb - 64));
                if (hit) f |= cbn_range(xa, xb);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) f |= __shfl_xor(f, o);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)f);
            const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(f >> 32));
            return word | ((unsigned long long)hi << 32) | lo;
        },
        [&](unsigned long long, int, int) {});
}

// The frame launch.  q [C, H, W], kv [C + Cv, H, W], bias [heads, 2 Wy - 1, 2 Wx - 1] f32 or NULL, out [Cv, H, W];
// mask: the frame's mask (the footprint launch's maskCopy); kvClear: kv's working mask behind a list of kv, else NULL.
// NTMAX >= the key tiles of a full cell (f16: rounded up to even) sizes the score registers and the LDS.
template <typename T, int NTMAX>
__global__ __launch_bounds__(256) void cbn_winattend_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                           const float* __restrict__ bias, T* __restrict__ out,
                                                           const unsigned long long* __restrict__ mask,
                                                           unsigned long long* __restrict__ kvClear, cbn_geo g, int wpr,
                                                           long units) {
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int KTOK = F16 ? 16 * NTMAX : 16 * (((NTMAX + 2) & ~3) + 1);      // tokens of a row of sK
    constexpr int QCH = F16 ? 32 : 4;                 // channels of one k-step of the scores
    constexpr int QREGS = CBN_MAXD / QCH;             // the Q fragment: 16 registers (f32), 2 x 4 (f16)
    constexpr int JI = (16 * NTMAX + 63) / 64;        // tokens of one lane
    using qfrag = typename std::conditional<F16, halfx8, float>::type;
    __shared__ __attribute__((aligned(16))) T sK[CBN_MAXD * KTOK];
    __shared__ __attribute__((aligned(16))) T sV[NTMAX * CBN_MAXD * 16];
    __shared__ float sBias[CBN_MAXBIAS];
    __shared__ int sTab[16 * NTMAX];                  // token j: row (2 Wx - 1) + column within the cell
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, gq = lane >> 4;
    const long HW = (long)g.H * g.W;
    const int bw = 2 * g.Wx - 1, nb = (2 * g.Wy - 1) * bw;
    for (long u = blockIdx.x; u < units; u += gridDim.x) {
        const int cell = (int)(u / g.heads), h = (int)(u - (long)cell * g.heads);
        const int cy = cell / g.ncx, cx = cell - cy * g.ncx;
        const int r0 = max(0, g.oy + cy * g.Wy), r1 = min(g.H, g.oy + (cy + 1) * g.Wy);
        const int xa = max(0, g.ox + cx * g.Wx), xb = min(g.W, g.ox + (cx + 1) * g.Wx);
        const int nr = r1 - r0, ncl = xb - xa, N = nr * ncl, NT = (N + 15) >> 4, NTE = F16 ? NT + (NT & 1) : NT;
        // the cell's segment of row r0 + lane of the frame's mask (every wave reads the same: uniform over the unit)
        unsigned seg = 0u;
        const int wi = xa >> 6, sh = xa & 63;
        if (lane < nr) {
            const unsigned long long* row = mask + (long)(r0 + lane) * wpr;
            const unsigned long long lo = row[wi];
            const unsigned long long hi = (sh != 0 && wi + 1 < wpr) ? row[wi + 1] : 0ull;
            seg = (unsigned)((lo >> sh) | (sh != 0 ? hi << (64 - sh) : 0ull)) & ((1u << ncl) - 1u);
        }
        if (__ballot(seg != 0u) == 0ull) continue;      // an idle unit
        if (kvClear && h == 0 && wave == 0 && lane < nr) {
            kvClear[(long)(r0 + lane) * wpr + wi] = 0ull;
            if (((xb - 1) >> 6) != wi) kvClear[(long)(r0 + lane) * wpr + wi + 1] = 0ull;
        }
        // ---- staging: lane (cs, jl) covers tokens jl + tl i of channel 4 cpw i' + cpw wave + cs
        const int NP = 16 * NT, NPE = 16 * NTE;
        const int tl = NPE <= 16 ? 16 : (NPE <= 32 ? 32 : 64), cpw = 64 / tl;
        const int jl = lane & (tl - 1), cs = lane / tl;
        int off[JI];                                   // the token's pixel, -1 for the tile tail
#pragma unroll
        for (int i = 0; i < JI; ++i) {
            const int j = jl + tl * i, rr = j / ncl;
            off[i] = j < N ? (r0 + rr) * g.W + xa + (j - rr * ncl) : -1;
        }
        __syncthreads();      // the unit before has been read
        {
            const T* kp = kv + (long)h * g.d * HW;
            const int kd = (g.d + QCH - 1) & ~(QCH - 1);
            for (int c = wave * cpw + cs; c < kd; c += 4 * cpw)
#pragma unroll
                for (int i = 0; i < JI; ++i) {
                    const int j = jl + tl * i;
                    if (j >= NP) continue;
                    const T val = (off[i] >= 0 && c < g.d) ? kp[(long)c * HW + off[i]] : T(0);
                    if constexpr (F16)
                        sK[((c >> 3) * KTOK + j) * 8 + (c & 7)] = val;
                    else
                        sK[c * KTOK + j] = val;
                }
            const T* vp = kv + ((long)g.C + (long)h * g.dv) * HW;
            const int vd = (g.dv + 15) & ~15;
            for (int c = wave * cpw + cs; c < vd; c += 4 * cpw)
#pragma unroll
                for (int i = 0; i < JI; ++i) {
                    const int j = jl + tl * i;
                    if (j >= NPE) continue;
                    sV[((j >> 4) * CBN_MAXD + c) * 16 + (j & 15)] =
                        (off[i] >= 0 && c < g.dv) ? vp[(long)c * HW + off[i]] : T(0);
                }
            if (g.hasBias) {
                for (int e = threadIdx.x; e < nb; e += 256) sBias[e] = bias[(long)h * nb + e];
                for (int j = threadIdx.x; j < NP; j += 256) {
                    const int rr = j / ncl;
                    sTab[j] = j < N ? rr * bw + (j - rr * ncl) : 0;
                }
            }
        }
        __syncthreads();
        const int nct = (g.dv + 15) >> 4;
        for (int qt = wave; qt < NT; qt += 4) {
            // query n of the tile (a tile tail computes the cell's last token again and stores nothing)
            const int tok = 16 * qt + n, ti = min(tok, N - 1), yi = ti / ncl, xi = ti - yi * ncl;
            const bool isq = tok < N;
            const long qoff = (long)(r0 + yi) * g.W + xa + xi;
            const unsigned rowseg = __shfl(seg, yi);      // (by every lane: a lane under a branch would read an idle one)
            const bool listed = isq & (bool)((rowseg >> xi) & 1u);
            // the Q fragment: channel on lane >> 4, query on lane & 15; zero beyond d and beyond the cell
            qfrag qf[QREGS];
            {
                const T* qp = q + (long)h * g.d * HW + qoff;
#pragma unroll
                for (int s = 0; s < QREGS; ++s) {
                    if constexpr (F16) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int c = 32 * s + 8 * gq + e;
                            qf[s][e] = (isq && c < g.d) ? qp[(long)c * HW] : cb_half(0);
                        }
                    } else {
                        const int c = 4 * s + gq;
                        qf[s] = (isq && c < g.d) ? qp[(long)c * HW] : 0.f;
                    }
                }
            }
            floatx4 S[NTMAX];
#pragma unroll
            for (int t = 0; t < NTMAX; ++t) S[t] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < QREGS; ++s) {
                if (s * QCH >= g.d) continue;
#pragma unroll
                for (int t = 0; t < NTMAX; ++t) {
                    if (t >= NT) continue;
                    if constexpr (F16) {
                        const halfx8 av = *(const halfx8*)&sK[((4 * s + gq) * KTOK + 16 * t + n) * 8];
                        S[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, qf[s], S[t], 0, 0, 0);
                    } else {
                        const float av = sK[(4 * s + gq) * KTOK + 16 * t + n];
                        S[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, qf[s], S[t], 0, 0, 0);
                    }
                }
            }
            // the softmax: lane (n, gq) holds keys 16 t + 4 gq + r of query n; a padding key is -inf by a select
            const int ci = (yi + g.Wy - 1) * bw + xi + g.Wx - 1;
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < NTMAX; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * t + 4 * gq + r;
                    const bool on = t < NT && j < N;
                    float s = S[t][r] * g.scale;
                    if (g.hasBias) {
                        const float b = sBias[on ? ci - sTab[j] : ci];      // (an index of the table either way)
                        s = s + (on ? b : 0.f);
                    }
                    s = on ? s : -INFINITY;
                    S[t][r] = s;
                    mx = fmaxf(mx, s);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float l = 0.f;
#pragma unroll
            for (int t = 0; t < NTMAX; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = S[t][r] > -INFINITY ? expf(S[t][r] - mx) : 0.f;
                    S[t][r] = p;
                    l = l + p;
                }
            l = l + __shfl_xor(l, 16);
            l = l + __shfl_xor(l, 32);
            floatx4 acc[CBN_MAXD / 16];                // channel 16 ct + 4 gq + r of query n
#pragma unroll
            for (int a = 0; a < CBN_MAXD / 16; ++a) acc[a] = floatx4{0.f, 0.f, 0.f, 0.f};
            if constexpr (F16) {
#pragma unroll
                for (int u2 = 0; u2 < NTMAX / 2; ++u2) {
                    if (2 * u2 >= NTE) continue;
                    halfx8 pb;      // K index 8 gq + e: tile 2 u2 + (e >> 2), key 4 gq + (e & 3)
#pragma unroll
                    for (int e = 0; e < 8; ++e) pb[e] = (cb_half)S[2 * u2 + (e >> 2)][e & 3];
#pragma unroll
                    for (int ct = 0; ct < CBN_MAXD / 16; ++ct) {
                        if (ct >= nct) continue;
                        const T* a0 = &sV[(2 * u2 * CBN_MAXD + 16 * ct + n) * 16 + 4 * gq];
                        const cbn_halfx4 lo = *(const cbn_halfx4*)a0;
                        const cbn_halfx4 hi = *(const cbn_halfx4*)(a0 + CBN_MAXD * 16);
                        const halfx8 av = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, pb, acc[ct], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < NTMAX; ++t) {
                    if (t >= NT) continue;
#pragma unroll
                    for (int ct = 0; ct < CBN_MAXD / 16; ++ct) {
                        if (ct >= nct) continue;
                        const floatx4 av = *(const floatx4*)&sV[(t * CBN_MAXD + 16 * ct + n) * 16 + 4 * gq];
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], S[t][r], acc[ct], 0, 0, 0);
                    }
                }
            }
            // C/D layout of the 16x16 MFMAs: query lane & 15, channel 4 (lane >> 4) + register
            if (listed) {
                T* o = out + (long)h * g.dv * HW + qoff;
#pragma unroll
                for (int a = 0; a < CBN_MAXD / 16; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ch = 16 * a + 4 * gq + r;
                        // one division, one rounding to the dtype
                        if (ch < g.dv) o[(long)ch * HW] = (T)(acc[a][r] / l);
                    }
            }
        }
    }
}

template <typename T>
void cbn_launch(const void* q, const void* kv, const float* bias, void* out, const uint64_t* mask, uint64_t* kvClear,
                const cbn_geo& g, int wpr, hipStream_t s) {
    const long units = (long)g.ncy * g.ncx * g.heads;
    const dim3 grid(cb_walk_grid(units)), block(256);
    const int full = min(g.Wy, g.H) * min(g.Wx, g.W);      // tokens of the largest cell
#define CBN_GO(NTMAX)                                                                                                  \
    hipLaunchKernelGGL((cbn_winattend_kernel<T, NTMAX>), grid, block, 0, s, (const T*)q, (const T*)kv, bias, (T*)out,   \
                       (const unsigned long long*)mask, (unsigned long long*)kvClear, g, wpr, units)
    if (full <= 64)
        CBN_GO(4);
    else if constexpr (sizeof(T) == 2)
        CBN_GO(10);
    else
        CBN_GO(9);
#undef CBN_GO
}

}  // namespace

int cbinfer_winattend_supported(const cbWinAttend* a, int C, int Cv, int H, int W) {
    if (!a || !(a->Wy >= 1 && a->Wy <= CBN_MAXW && a->Wx >= 1 && a->Wx <= CBN_MAXW && a->Wy * a->Wx <= CBN_MAXN)) return 0;
    if (!(a->sy >= 0 && a->sy < a->Wy && a->sx >= 0 && a->sx < a->Wx)) return 0;
    if (!(a->heads >= 1 && a->heads <= CBN_MAXHEADS && C >= 1 && Cv >= 1 && H >= 1 && W >= 1)) return 0;
    if (C % a->heads || Cv % a->heads || C / a->heads > CBN_MAXD || Cv / a->heads > CBN_MAXD) return 0;
    if (!(a->hasBias == 0 || a->hasBias == 1)) return 0;
    if (!(a->scale == a->scale && fabsf(a->scale) <= 3.0e38f)) return 0;      // (finite)
    // (a list addresses a pixel with an int32; C + Cv <= 2 x 64 x 64 planes is within the other operators' limit)
    return (long)H * W < (1l << 31);
}

int cbinfer_cbwinattend_forward(const void* q, const void* kv, const float* positionBias, void* outputState,
                                const uint64_t* maskQ, const int32_t* listQ, int capQ, const int32_t* countQ,
                                const uint64_t* maskKV, const int32_t* listKV, int capKV, const int32_t* countKV,
                                uint64_t* kvBits, uint64_t* bits, uint64_t* maskCopy, int C, int Cv, int H, int W,
                                const cbWinAttend* attend, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    const cbw_forms f = {maskQ, listQ, capQ, countQ, maskKV, listKV, capKV, countKV, kvBits, bits, maskCopy};
    CB_REQUIRE(q && kv && outputState && outputState != q && outputState != kv && q != kv);
    CB_REQUIRE(cbw_forms_ok(f));
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_winattend_supported(attend, C, Cv, H, W));
    CB_REQUIRE((attend->hasBias != 0) == (positionBias != nullptr));
    cbn_geo g;
    g.C = C, g.Cv = Cv, g.H = H, g.W = W, g.heads = attend->heads, g.d = C / attend->heads, g.dv = Cv / attend->heads;
    g.Wy = attend->Wy, g.Wx = attend->Wx;
    g.oy = attend->sy > 0 ? attend->sy - attend->Wy : 0, g.ox = attend->sx > 0 ? attend->sx - attend->Wx : 0;
    g.ncy = (H - g.oy + g.Wy - 1) / g.Wy, g.ncx = (W - g.ox + g.Wx - 1) / g.Wx;
    g.hasBias = attend->hasBias, g.scale = attend->scale;
    const hipStream_t s = (hipStream_t)stream;
    cbw_frame fr;
    int st = cbw_lists_to_bits(f, H, W, stream, &fr);
    if (st != CB_OK) return st;
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    hipLaunchKernelGGL(cbn_footprint_kernel, dim3(cb_walk_grid(words)), dim3(256), 0, s,
                       (const unsigned long long*)fr.mA, (const unsigned long long*)fr.mB, fr.all,
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, g, wpr);
    st = cb_launch_status();
    if (st != CB_OK) return st;
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbn_launch<decltype(t)>(q, kv, positionBias, outputState, maskCopy, fr.bList ? kvBits : nullptr, g, wpr, s);
    });
    return cb_launch_status();
}
