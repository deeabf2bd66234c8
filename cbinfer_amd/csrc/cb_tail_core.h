// The arithmetic of the fused 1x1 tail (cb_tail.hip) for ONE tile of CB_TAIL_PX changed pixels whose input columns
// are (being) staged in LDS -- shared by cb_tail1x1_kernel, which gathers them from the producing layer's output,
// and cbs_reduce_tail_kernel (cb_split.hip), which makes them from the partial tiles of a split contraction: one
// body, so both give the same bits.
#pragma once
#include "cb_common.h"

#ifndef CB_TAIL_STAMP
#define CB_TAIL_STAMP(i)
#endif

#define CB_TAIL_PX 16
#define CB_TAIL_MAXW 8          // row blocks of 16 hidden channels per workgroup: R = ceil(C1/16) <= 8  -> C1 <= 128
#define CB_TAIL_MAXT 1024       // threads of the widest workgroup: R row blocks x S chain sets = 16 waves

// The workgroup is R x S waves: wave (r, c) = (wave % R, wave / R) owns the 16 hidden rows of block r and, of the first
// layer's four accumulation chains (fragment group i feeds chain i % 4), the 4/S chains 4/S c .. 4/S c + 4/S - 1: the
// chains share no data until they are summed, so each runs in a wave of its own instead of one wave walking all four.
// S = 4 for up to four row blocks, 2 for up to eight (16 waves at most).  The chain sets meet in LDS, in the X tile's
// space (its last reader is the first layer), so no LDS is added: S is halved while the last chain set would have no
// fragment group to multiply (fewer than four groups) or the partial accumulators of the sets c > 0 -- R KB per chain
// that received anything -- do not fit into the tile (C0P/16 KB): narrow inputs under wide hidden layers.
__host__ __device__ inline int cb_tail_chain_sets(int C0, int C1) {
    const int groups = (C0 + 15) / 16, R = (C1 + 15) / 16, live = groups < 4 ? groups : 4;
    int S = R <= 4 ? 4 : 2;
    while (S > 1 && !(live > 4 - 4 / S && (live - 4 / S) * R <= groups)) S >>= 1;
    return S;
}

// dynamic LDS of a tail workgroup: Xs[C0P][16] | Hs[16 R][17] | W2s[C2][C1] | b2s[C2]
struct CbTailLds {
    float *Xs, *Hs, *W2s, *b2s;
};
__device__ __forceinline__ CbTailLds cb_tail_lds(float* sm, int C0P, int C1, int C2) {
    CbTailLds l;
    l.Xs = sm;
    l.Hs = sm + (long)C0P * CB_TAIL_PX;
    l.W2s = l.Hs + (C1 + 15) / 16 * 16 * (CB_TAIL_PX + 1);
    l.b2s = l.W2s + C2 * C1;
    return l;
}
__host__ __device__ inline size_t cb_tail_lds_bytes(int C0, int C1, int C2) {
    const int C0P = (C0 + 15) / 16 * 16;
    const int waves = (C1 + 15) / 16;
    return ((size_t)C0P * CB_TAIL_PX + (size_t)waves * 16 * (CB_TAIL_PX + 1) + (size_t)C2 * C1 + C2) * 4;
}

// X[c][px] of one tile gathered from a [C0][HW] map: thread -> (px = t % 16, channels c00 + u cstep, c00 = t / 16,
// cstep = threads / 16); 16 neighbouring lanes read the 16 pixels of one channel plane (contiguous where the changed
// pixels are).  U loads in flight per lane, U = what a thread has to fetch (a wide workgroup on few channels would
// clamp the rest to copies of its last one), UMAX at most.  Never predicated -- a predicated load is a branch of its
// own, sixteen of them sixteen round trips: clamped addresses, predicated uses.
template <int U>
__device__ __forceinline__ void cb_tail_gather_u(float* Xs, const float* __restrict__ src, int HW, int pixLd, bool valid,
                                                 int C0, int C0P, int c00, int px, int cstep) {
    for (int c0 = c00; c0 < C0P; c0 += U * cstep) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = src[(long)min(c0 + u * cstep, C0 - 1) * HW + pixLd];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * cstep;
            if (c < C0P) Xs[c * CB_TAIL_PX + px] = (valid && c < C0) ? v[u] : 0.f;
        }
    }
}
// (UMAX: sixteen for a workgroup of up to eight waves, eight under the 128 registers of a wider one)
template <int UMAX>
__device__ __forceinline__ void cb_tail_gather(float* Xs, const float* __restrict__ src, int HW, int pixLd, bool valid,
                                               int C0, int C0P, int c00, int px, int cstep) {
    const int per = (C0P + cstep - 1) / cstep;      // (uniform)
    if (per <= 1) cb_tail_gather_u<1>(Xs, src, HW, pixLd, valid, C0, C0P, c00, px, cstep);
    else if (per <= 2) cb_tail_gather_u<2>(Xs, src, HW, pixLd, valid, C0, C0P, c00, px, cstep);
    else if (per <= 4) cb_tail_gather_u<4>(Xs, src, HW, pixLd, valid, C0, C0P, c00, px, cstep);
    else if (per <= 8 || UMAX == 8) cb_tail_gather_u<8>(Xs, src, HW, pixLd, valid, C0, C0P, c00, px, cstep);
    else cb_tail_gather_u<16>(Xs, src, HW, pixLd, valid, C0, C0P, c00, px, cstep);
}

// What a wave needs from memory for every tile it evaluates, the same for all of them: of the first 16 fragment groups
// of its 16 rows of W1 (all of them up to 256 input channels) the 16/S its chains multiply, and its rows' biases.
// Slot k of wave (r, c) holds fragment group cb_tail_group<S>(k, c): its chains' groups in rising order.
template <int S>
struct CbTailPre {
    floatx4 a[16 / S];
    float b1v[4];
};
template <int S>
__device__ __forceinline__ int cb_tail_group(int k, int c) {
    constexpr int PER = 4 / S;
    return 4 * (k / PER) + PER * c + k % PER;
}
template <int S>
__device__ __forceinline__ void cb_tail_preload(CbTailPre<S>& P, const float* __restrict__ w1p,
                                                const float* __restrict__ b1, int C0P, int C1) {
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int R = (C1 + 15) / 16, c = S == 1 ? 0 : wave / R, r = wave - c * R;
    const int groups = C0P / 16;
    const floatx4* ap = (const floatx4*)w1p + ((long)r * groups) * 64 + lane;
#pragma unroll
    for (int k = 0; k < 16 / S; ++k) P.a[k] = ap[(long)min(cb_tail_group<S>(k, c), groups - 1) * 64];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int m = 16 * r + 4 * (lane >> 4) + q;
        P.b1v[q] = m < C1 ? b1[m] : 0.f;
    }
}

// Called by every thread of the workgroup once its part of the X tile is WRITTEN to l.Xs (the barrier that makes the
// tile complete is inside).  s_pix[px]: pixel index or -1.
template <int S>
__device__ __forceinline__ void cb_tail_tile(const CbTailLds& l, const int* s_pix, const CbTailPre<S>& P,
                                             const float* __restrict__ w1p, float* out, int C0P, int C1, int C2, int HW,
                                             int relu1, int relu2) {
    constexpr int PER = 4 / S, NA = 16 / S;
    const int t = threadIdx.x, NT = blockDim.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int R = (C1 + 15) / 16, c = S == 1 ? 0 : wave / R, r = wave - c * R, NT0 = 64 * R;
    float* Xs = l.Xs;
    float* Hs = l.Hs;
    const float* W2s = l.W2s;
    const float* b2s = l.b2s;
    // H tile of row block r: rows 16 r .. +15, cols = 16 px.  A: lane holds W1[16r + l%16][4s + l/16],
    // B: lane holds X[4s + l/16][l%16].  (Fetched one by one in the MFMA loop the weight fragments cost sixteen
    // L2 round trips per tile: 15.8 us per launch in the frame, round 2.)
    // Four accumulation chains (fragment group i feeds chain i % 4), summed at the end: a single chain of 4 C0P/16
    // dependent matrix instructions, each waiting for its predecessor and for an LDS read, took 2 us of a 12 us launch.
    // This wave runs PER of them: acc[e] is chain PER c + e.
    floatx4 acc[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) acc[e] = floatx4{0.f, 0.f, 0.f, 0.f};
    const floatx4* ap = (const floatx4*)w1p + ((long)r * (C0P / 16)) * 64 + lane;
    const float* bp = Xs + (lane >> 4) * CB_TAIL_PX + (lane & 15) + 16 * PER * c * CB_TAIL_PX;
    const int groups = C0P / 16;
    __syncthreads();   // the X tile is complete
    CB_TAIL_STAMP(4);
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int il = cb_tail_group<S>(k, 0);      // (the group's distance from the wave's first one)
        if (il + PER * c < groups) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[k % PER] = __builtin_amdgcn_mfma_f32_16x16x4f32(P.a[k][j], bp[(16 * il + 4 * j) * CB_TAIL_PX], acc[k % PER],
                                                                    0, 0, 0);
        }
        if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // (at most 16 LDS operands requested ahead)
    }
    for (int g0 = 16; g0 < groups; g0 += 16) {      // (more than 256 input channels)
        floatx4 a[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) a[k] = ap[(long)min(g0 + cb_tail_group<S>(k, c), groups - 1) * 64];
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int il = cb_tail_group<S>(k, 0);
            if (g0 + il + PER * c < groups) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[k % PER] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k][j], bp[(16 * (g0 + il) + 4 * j) * CB_TAIL_PX],
                                                                        acc[k % PER], 0, 0, 0);
            }
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
    floatx4 accs;
    if constexpr (S == 1) {
        accs = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    } else {
        // the chain sets meet in the X tile's space: chain a >= PER of row block r at [(a - PER) R + r][lane]; a chain
        // without a fragment group (fewer than four groups) is the zero it started from
        const int live = min(4, groups);
        floatx4* Pt = (floatx4*)Xs;
        __syncthreads();   // every wave is past its last read of the X tile
        if (c > 0) {
#pragma unroll
            for (int e = 0; e < PER; ++e)
                if (PER * c + e < live) Pt[((PER * c + e - PER) * R + r) * 64 + lane] = acc[e];
        }
        __syncthreads();
        floatx4 ch[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (a < PER) ch[a] = acc[a];
            else ch[a] = (c == 0 && a < live) ? Pt[((a - PER) * R + r) * 64 + lane] : floatx4{0.f, 0.f, 0.f, 0.f};
        }
        accs = (ch[0] + ch[1]) + (ch[2] + ch[3]);
    }
    // C/D map of the 16x16 tile: col = lane%16, row = 4*(lane/16) + q
    if (c == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = 16 * r + 4 * (lane >> 4) + q;
            float v = accs[q] + P.b1v[q];
            if (relu1) v = v <= 0.f ? 0.f : v;
            Hs[m * (CB_TAIL_PX + 1) + (lane & 15)] = v;
        }
    }
    CB_TAIL_STAMP(5);
    __syncthreads();
    CB_TAIL_STAMP(6);
    // second layer: out[c2][px] = b2[c2] + sum_j W2[c2][j] * H[j][px], on the 64 R threads of the chain set 0 (the
    // workgroup before it had chain sets: the deal below is part of the bits).  With threads to spare the hidden
    // channels are dealt over PARTS of them (part k: the k-th quarter, ...), the partial sums meet in LDS (the X tile's
    // space: its last reader was the first layer) and are added in part order.
    const int outs = C2 * CB_TAIL_PX;
    int parts = 1;
    while (parts < 4 && 2 * parts * outs <= NT0 && 2 * parts * outs <= C0P * CB_TAIL_PX && C1 % (2 * parts) == 0) parts *= 2;
    float* Ps = Xs;
    const int o = t % outs, part = t / outs;
    const int c2 = o >> 4, p2 = o & 15;
    if (t < NT0 && part < parts) {
        const int j0 = part * (C1 / parts), j1 = j0 + C1 / parts;
        float v = part == 0 ? b2s[c2] : 0.f;
        const float* wr = W2s + c2 * C1;
#pragma unroll 8
        for (int j = j0; j < j1; ++j) v = fmaf(wr[j], Hs[j * (CB_TAIL_PX + 1) + p2], v);
        if (parts > 1) Ps[part * outs + o] = v;
        if (parts == 1) {
            const int pix = s_pix[p2];
            if (relu2) v = v <= 0.f ? 0.f : v;
            if (pix >= 0) out[(long)c2 * HW + pix] = v;
        }
    }
    if (parts > 1) {
        __syncthreads();
        if (t < outs) {
            float v = Ps[o];
            for (int k = 1; k < parts; ++k) v += Ps[k * outs + o];
            const int pix = s_pix[p2];
            if (relu2) v = v <= 0.f ? 0.f : v;
            if (pix >= 0) out[(long)c2 * HW + pix] = v;
        }
    }
    for (int o2 = NT0 + t; o2 < outs; o2 += NT) {      // (more outputs than 64 R threads: the plain form for the rest)
        const int c3 = o2 >> 4, p3 = o2 & 15;
        const int pix = s_pix[p3];
        if (pix < 0) continue;
        float v = b2s[c3];
        const float* wr = W2s + c3 * C1;
#pragma unroll 8
        for (int j = 0; j < C1; ++j) v = fmaf(wr[j], Hs[j * (CB_TAIL_PX + 1) + p3], v);
        if (relu2) v = v <= 0.f ? 0.f : v;
        out[(long)c3 * HW + pix] = v;
    }
}
