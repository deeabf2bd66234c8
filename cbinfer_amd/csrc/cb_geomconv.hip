// General-geometry change-based convolution for gfx950: stride, dilation, free zero padding, even filter sizes,
// optional bias.  The unit-geometry kernels (cb_detect.hip, cb_conv.hip) assume that the input map IS the output map
// and that the filter is centred; here the two maps differ:
//   input map  Hi x Wi, filter kH x kW, stride (sH, sW), padding (pH, pW), dilation (dH, dW)
//   output map Ho = (Hi + 2 pH - dH (kH-1) - 1) / sH + 1, Wo likewise
// Two launches per frame, no im2col matrix and no host round trip:
//   cbg_detect_kernel  per-pixel change on the INPUT map (component a1's rule), state refresh, and the exact footprint
//                      of the changed pixels -- output (oy, ox) is hit iff one of its taps (oy sH - pH + ky dH,
//                      ox sW - pW + kx dW) is a changed input pixel -- ORed into a row-padded bit mask of the OUTPUT
//                      map, in the frame-mask protocol (two alternating masks + parity, cbinfer_frame_mask_bytes);
//   cbg_conv_kernel    derives the ascending change list from that mask by itself (or takes a list), gathers the taps
//                      of 64 listed output pixels per tile through the k -> tap table, contracts them with the filter
//                      bank on the MFMA units (f16; f32 as bf16 triples, six products; or the exact f32 MFMA), adds the
//                      bias, applies the ReLU and scatters into the output planes.  A short list is split along k over
//                      idle workgroups; the slices are summed in slice order by the last one to arrive.
// Entry-point contracts: include/cbinfer_hip.h, "general geometry".
#include "cb_common.h"
#include "cb_geom_stage.h"

namespace {

#define CBG_MAX_K 7      // filter size per axis
#define CBG_MAX_S 4      // stride per axis
#define CBG_MAX_D 8      // dilation per axis
#define CBG_MAX_P 64     // padding per axis
#define CBG_BM 64        // output channels per tile
#define CBG_BN 64        // listed pixels per tile
#define CBG_BK 32        // k-depth per LDS stage
#define CBG_GRID 512     // persistent grid of the contraction (2 workgroups per CU of an MI355X)
#define CBG_SKMAX 8      // most k-slices per tile
#define CBG_SLAB (CBG_BM * CBG_BN)

int cbg_geom_status(const cbGeom* g) {
    if (!g) return CB_ERR_BADARG;
    if (g->kH < 1 || g->kW < 1 || g->sH < 1 || g->sW < 1 || g->dH < 1 || g->dW < 1 || g->pH < 0 || g->pW < 0)
        return CB_ERR_BADARG;
    if (g->kH > CBG_MAX_K || g->kW > CBG_MAX_K || g->sH > CBG_MAX_S || g->sW > CBG_MAX_S || g->dH > CBG_MAX_D ||
        g->dW > CBG_MAX_D || g->pH > CBG_MAX_P || g->pW > CBG_MAX_P)
        return CB_ERR_UNSUPPORTED;
    return CB_OK;
}

int cbg_out_size(int Hi, int Wi, const cbGeom* g, int* Ho, int* Wo) {
    const int st = cbg_geom_status(g);
    if (st != CB_OK) return st;
    if (Hi < 1 || Wi < 1) return CB_ERR_BADARG;
    const int nh = Hi + 2 * g->pH - g->dH * (g->kH - 1) - 1, nw = Wi + 2 * g->pW - g->dW * (g->kW - 1) - 1;
    if (nh < 0 || nw < 0) return CB_ERR_BADARG;      // (the dilated filter does not fit the padded map)
    *Ho = nh / g->sH + 1;
    *Wo = nw / g->sW + 1;
    return CB_OK;
}

int cbg_kpad(int K) { return (K + CBG_BM - 1) / CBG_BM * CBG_BM; }
int cbg_ckkpad(int Ckk) { return (Ckk + CBG_BK - 1) / CBG_BK * CBG_BK; }

// ---------------------------------------------------------------------------------------------
// weight preparation: W[KP][CkkP] in the tensors' element type (k contiguous, zero padded), then the k -> tap table:
//   off[k]  = byte offset of tap (c, ky, kx) relative to the BASE pixel (oy sH, ox sW) of the input map
//   dydx[k] = (dx << 16) | (dy & 0xffff) with dy = ky dH - pH, dx = kx dW - pW (the border test against Hi, Wi)
// The padded tail k >= Ckk gets dy = dx = -32768: outside every map (either one alone is not -- a base pixel at row
// 32768 or beyond brings the tap back inside a map that tall; both at once would need 2^30 pixels, which
// cbinfer_geom_prep_weights refuses).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cbg_prep_kernel(const T* __restrict__ w, T* __restrict__ wp, int K, int Ckk,
                                                      int KP, int CkkP, int Hi, int Wi, cbGeom g) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < CkkP) {
        int* tab = (int*)(wp + (long)KP * CkkP);
        const int k = (int)e;
        if (k >= Ckk) {
            tab[k] = 0;
            tab[CkkP + k] = (int)0x80008000u;
        } else {
            const int c = k / (g.kH * g.kW), r = k % (g.kH * g.kW);
            const int dy = (r / g.kW) * g.dH - g.pH, dx = (r % g.kW) * g.dW - g.pW;
            tab[k] = (c * Hi * Wi + dy * Wi + dx) * (int)sizeof(T);
            tab[CkkP + k] = (dx << 16) | (dy & 0xffff);
        }
    }
    if (e >= (long)KP * CkkP) return;
    const int k = (int)(e % CkkP), m = (int)(e / CkkP);
    wp[e] = (m < K && k < Ckk) ? w[(long)m * Ckk + k] : T(0);
}

// ---------------------------------------------------------------------------------------------
// detection: one workgroup = one 64-pixel row segment of the INPUT map x all channels (1 to 16 waves by the channel
// count; wave g scans channels g, g+G, ...; one coalesced row segment per wave load), ballots OR-reduced through LDS as in cb_detect_kernel.
//   update 1: in[:, p] -> state[:, p] at the changed pixels only (feedback);  2: wherever the values differ at all.
// The footprint is built by wave 0 with word arithmetic: for every output word the segment can reach, lane j owns
// output column ox = 64 w + j and tests the kW input bits its taps fall on; a ballot makes the word, which is ORed into
// the kH output rows the input row feeds (at most one per ky: oy = (y + pH - ky dH) / sH where that divides).  With a
// stride the 64 input bits land on every sW-th tap phase -- the lanes' reads of `m` are that compression.  A changed
// pixel no tap reaches (1x1 stride 2, odd coordinates) leaves no bit but still refreshes the state.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void cbg_detect_kernel(const T* __restrict__ in, T* state,
                                                        unsigned long long* __restrict__ masks, long maskWords, int C,
                                                        int Hi, int Wi, int Ho, int Wo, int wprO, cbGeom g, float thf,
                                                        int update) {
    unsigned long long* bits = masks;
    if (*(const int*)(masks + 2 * maskWords)) bits += maskWords;      // the mask the parity selects
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, G = blockDim.x >> 6;
    const int tx = blockIdx.x, y = blockIdx.y;
    const int x = tx * 64 + lane;
    const bool valid = x < Wi;
    const long HW = (long)Hi * Wi, p = (long)y * Wi + x;
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
    if (m == 0) return;      // uniform over the workgroup

    if (update == 1 && ((m >> lane) & 1ull))
        for (int c = wv; c < C; c += G) state[(long)c * HW + p] = in[(long)c * HW + p];
    if (wv != 0) return;

    const int x0 = tx * 64;
    const int lo = x0 + g.pW - (g.kW - 1) * g.dW;
    const int oxLo = lo <= 0 ? 0 : (lo + g.sW - 1) / g.sW;
    const int oxHi = min((x0 + 63 + g.pW) / g.sW, Wo - 1);
    if (oxLo > oxHi) return;
    // lane r < kH: the output row that reads this input row with filter row r
    const int ny = y + g.pH - lane * g.dH;
    const int oy = ny / g.sH;
    const bool rowOk = lane < g.kH && ny >= 0 && ny % g.sH == 0 && oy < Ho;
    for (int w = oxLo >> 6; w <= (oxHi >> 6); ++w) {
        const int ox = w * 64 + lane;
        bool bit = false;
        if (ox < Wo)
            for (int kx = 0; kx < g.kW; ++kx) {
                const int bpos = ox * g.sW - g.pW + kx * g.dW - x0;
                if ((unsigned)bpos < 64u) bit |= (m >> bpos) & 1ull;
            }
        const unsigned long long word = __ballot(bit);
        if (word && rowOk) atomicOr(&bits[(long)oy * wprO + w], word);
    }
}

// ---------------------------------------------------------------------------------------------
// contraction
// ---------------------------------------------------------------------------------------------
struct GeomConvParams {
    const void* W;       // prepared weights [KP][CkkP]
    const int* tab;      // tap table behind them
    const void* src;     // the map the gather reads [C, Hi, Wi]
    const void* bias;    // [K] or null
    void* out;           // [K, Ho, Wo]
    const int32_t* list;               // list mode: ascending flat output pixels ...
    const int32_t* countDev;           // ... and their number on the device (null: nHost)
    int nHost;
    unsigned long long* frameMasks;    // mask mode: [2][maskWords] masks, {parity, done}, mask copy
    long maskWords;
    int wpr;
    int32_t* listOut;                  // mask mode: the list and its length as a by-product
    int32_t* countOut;
    float* slabs;                      // split-k workspace (null: no split) ...
    int* tickets;                      // ... and arrival counters, zero between launches
    int K, KP, CkkP, Hi, Wi, Ho, Wo, sH, sW, relu;
};

// T: element type of the tensors; ARITH: CB_F16 (T = half), CB_F32S or CB_F32 (T = float).
// 256 threads = 2 x 2 waves, one 32 x 32 MFMA tile each (output channel in the accumulator registers, listed pixel on
// the lane: a store instruction of the epilogue writes 32 pixels of one output plane).  Per stage of 32 k every thread
// loads 8 consecutive k of one weight row (16 / 32 bytes) and gathers 8 consecutive k of one pixel -- a wave's k are
// uniform, so its taps come from the table by scalar loads --; the loads of stage s+1 are in flight while the MFMAs of
// stage s run (two LDS buffers, one barrier per stage).
template <typename T, int ARITH>
__global__ __launch_bounds__(256) void cbg_conv_kernel(GeomConvParams p) {
    __shared__ CbgStage<ARITH> sA[2], sB[2];
    __shared__ int sPre[257];
    __shared__ int sList[CBG_BN];
    __shared__ int sLast;
    __shared__ int sWave[4];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int G = gridDim.x, HWo = p.Ho * p.Wo;

    // ---- the change list: from the frame mask (ascending by construction) or as given
    int N;
    const unsigned long long* cur = nullptr;
    const long words = p.maskWords;
    const int chunk = (int)((words + 255) / 256);
    if (p.frameMasks) {
        N = cbg_list_from_mask(p.frameMasks, words, chunk, p.wpr, p.Wo, p.listOut, p.countOut, sPre, sWave, cur);
    } else {
        N = p.countDev ? min(*p.countDev, p.nHost) : p.nHost;
        N = max(0, min(N, HWo));
    }
    if (N == 0) return;

    // ---- work items: (pixel tile, channel tile, k-slice)
    const int tilesN = (N + CBG_BN - 1) / CBG_BN, tilesM = p.KP / CBG_BM, stages = p.CkkP / CBG_BK;
    const int base = tilesN * tilesM;
    int SK = 1;
    if (p.slabs && base < G) SK = max(1, min(min(G / base, CBG_SKMAX), stages));
    const int items = base * SK;      // (SK > 1: items <= G, one item and one slab per workgroup)

    const int gn = t & 63, gk = wave * 8;      // gather: pixel row, first k of the stage
    const int am = t >> 2, ak = (t & 3) * 8;   // weights: channel row, first k of the stage
    const int wm = wave & 1, wn = wave >> 1;
    const T* src = (const T*)p.src;

    for (int item = blockIdx.x; item < items; item += G) {
        const int slice = item % SK, tm = (item / SK) % tilesM, tn = item / (SK * tilesM);
        const int s0 = (int)((long)stages * slice / SK), s1 = (int)((long)stages * (slice + 1) / SK);
        __syncthreads();
        if (t < CBG_BN) {
            const int q = tn * CBG_BN + t;
            sList[t] = q < N ? cbg_list_entry(q, cur, sPre, words, chunk, p.wpr, p.Wo, p.list, HWo) : -1;
        }
        __syncthreads();

        const int pix = sList[gn];
        const int oy = pix < 0 ? 0 : pix / p.Wo, ox = pix < 0 ? 0 : pix % p.Wo;
        const int iy0 = oy * p.sH, ix0 = ox * p.sW;
        const char* pbase = (const char*)(src + (long)iy0 * p.Wi + ix0);
        const T* wrow = (const T*)p.W + ((long)tm * CBG_BM + am) * p.CkkP + ak;

        T ra[8], rb[8];
        auto load = [&](int s) {
            const T* wsrc = wrow + (long)s * CBG_BK;
            if constexpr (sizeof(T) == 2) {
                const uint4 v = *(const uint4*)wsrc;
                __builtin_memcpy(ra, &v, 16);
            } else {
                const float4 v0 = *(const float4*)wsrc, v1 = *(const float4*)(wsrc + 4);
                __builtin_memcpy(ra, &v0, 16);
                __builtin_memcpy(ra + 4, &v1, 16);
            }
            const int* tab = p.tab + s * CBG_BK + gk;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int off = tab[i], dd = tab[p.CkkP + i];
                const int dy = (short)(dd & 0xffff), dx = dd >> 16;
                const bool inb = pix >= 0 && (unsigned)(iy0 + dy) < (unsigned)p.Hi && (unsigned)(ix0 + dx) < (unsigned)p.Wi;
                rb[i] = inb ? *(const T*)(pbase + off) : T(0);
            }
        };

        floatx16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        // two LDS buffers, one barrier per stage: the loads of stage s+1 fly during the MFMAs of stage s and land in
        // the other buffer behind them (whose last readers passed the previous barrier)
        if (s0 < s1) {
            load(s0);
            sA[0].put(am, ak, ra);
            sB[0].put(gn, gk, rb);
        }
        __syncthreads();
        for (int s = s0; s < s1; ++s) {
            const int cb = (s - s0) & 1;
            if (s + 1 < s1) load(s + 1);
            acc = cbg_mfma_stage<ARITH>(sA[cb], sB[cb], wm * 32 + (lane & 31), wn * 32 + (lane & 31), lane, acc);
            if (s + 1 < s1) {
                sA[cb ^ 1].put(am, ak, ra);
                sB[cb ^ 1].put(gn, gk, rb);
            }
            __syncthreads();
        }

        // ---- split-k: partial tiles to the workspace, summed in slice order by the last workgroup to arrive.  The
        // hand-off needs no agent-scope release (an L2 write-back per workgroup, which serialises the launch): every
        // slab store is write-through (sc1: an agent-scope relaxed atomic store) and drained before the workgroup's
        // ticket, every slab load is an sc1 load behind the reducer's acquire (MI355X_MICROARCH.md, "Inter-workgroup
        // visibility").
        if (SK > 1) {
            // (slab = [4 waves][4 register quads][64 lanes] float4: 16 bytes per lane, 1 KB per wave instruction)
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            const __amdgpu_buffer_rsrc_t srsrc =
                __builtin_amdgcn_make_buffer_rsrc((void*)p.slabs, 0, CBG_GRID * CBG_SLAB * 4, 0x00020000);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 f = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f), srsrc,
                                                       (item * (CBG_SLAB / 4) + (wave * 4 + q) * 64 + lane) * 16, 0,
                                                       16 /* sc1 */);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            int* ticket = p.tickets + (tn * tilesM + tm);
            if (t == 0) {
                const int old = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == SK - 1) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                sLast = old == SK - 1;
            }
            __syncthreads();
            if (!sLast) continue;
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = 0.f;
            for (int sl = 0; sl < SK; ++sl)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                        srsrc, ((item - slice + sl) * (CBG_SLAB / 4) + (wave * 4 + q) * 64 + lane) * 16, 0, 16 /* sc1 */));
                    acc[4 * q] += f.x, acc[4 * q + 1] += f.y, acc[4 * q + 2] += f.z, acc[4 * q + 3] += f.w;
                }
        }

        // ---- bias, ReLU, scatter
        const int opix = sList[wn * 32 + (lane & 31)];
        if (opix >= 0) {
            T* out = (T*)p.out;
            const T* bias = (const T*)p.bias;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int m = tm * CBG_BM + wm * 32 + (j >> 2) * 8 + (lane >> 5) * 4 + (j & 3);
                if (m < p.K) {
                    float v = acc[j] + (bias ? (float)bias[m] : 0.f);
                    if (p.relu) v = v <= 0.f ? 0.f : v;
                    out[(long)m * HWo + opix] = (T)v;
                }
            }
        }
    }
}

int cbg_launch_conv(const GeomConvParams& p, int dtype, hipStream_t s) {
    dim3 grid(CBG_GRID), block(256);
    if (dtype == CB_F16)
        hipLaunchKernelGGL((cbg_conv_kernel<cb_half, CB_F16>), grid, block, 0, s, p);
    else if (dtype == CB_F32S)
        hipLaunchKernelGGL((cbg_conv_kernel<float, CB_F32S>), grid, block, 0, s, p);
    else
        hipLaunchKernelGGL((cbg_conv_kernel<float, CB_F32>), grid, block, 0, s, p);
    return cb_launch_status();
}

}  // namespace

extern "C" {

int cbinfer_geom_out_size(int Hi, int Wi, const cbGeom* geom, int* Ho, int* Wo) {
    CB_REQUIRE(Ho && Wo);
    return cbg_out_size(Hi, Wi, geom, Ho, Wo);
}

long cbinfer_geom_prepared_weights_bytes(int K, int C, const cbGeom* geom, int dtype) {
    if (cbg_geom_status(geom) != CB_OK || K < 1 || C < 1) return 0;
    const long KP = cbg_kpad(K), CkkP = cbg_ckkpad(C * geom->kH * geom->kW);
    return KP * CkkP * (dtype == CB_F16 ? 2 : 4) + CkkP * 8;
}

long cbinfer_geom_workspace_bytes(void) { return (long)CBG_GRID * CBG_SLAB * 4 + (long)CBG_GRID * 4; }

int cbinfer_geom_prep_weights(const void* weight, void* prepared, int K, int C, int Hi, int Wi, const cbGeom* geom,
                              int dtype, cbStream_t stream) {
    CB_REQUIRE(weight && prepared && K > 0 && C > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16 || dtype == CB_F32S);
    int Ho, Wo;
    const int st = cbg_out_size(Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    if ((long)C * Hi * Wi * 4 >= (1l << 30)) return CB_ERR_UNSUPPORTED;      // (tap offsets are 32-bit byte offsets)
    const int Ckk = C * geom->kH * geom->kW, KP = cbg_kpad(K), CkkP = cbg_ckkpad(Ckk);
    dim3 grid(cb_div_up((long)KP * CkkP, 256)), block(256);
    if (dtype == CB_F16)
        hipLaunchKernelGGL(cbg_prep_kernel<cb_half>, grid, block, 0, (hipStream_t)stream, (const cb_half*)weight,
                           (cb_half*)prepared, K, Ckk, KP, CkkP, Hi, Wi, *geom);
    else
        hipLaunchKernelGGL(cbg_prep_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)weight,
                           (float*)prepared, K, Ckk, KP, CkkP, Hi, Wi, *geom);
    return cb_launch_status();
}

int cbinfer_change_detection_geom(const void* input, void* state, uint64_t* frameMasks, int C, int Hi, int Wi,
                                  const cbGeom* geom, float threshold, int updateInputState, int dtype,
                                  cbStream_t stream) {
    CB_REQUIRE(input && state && frameMasks && C > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(updateInputState >= 0 && updateInputState <= 2);
    int Ho, Wo;
    const int st = cbg_out_size(Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    if (Hi > 65535) return CB_ERR_UNSUPPORTED;
    const int wprO = cbinfer_mask_words_per_row(Wo);
    const long words = cbinfer_mask_words(Ho, Wo);
    dim3 grid(cb_div_up(Wi, 64), Hi), block(64 * (C >= 32 ? 16 : C >= 8 ? 8 : C >= 4 ? 4 : C));      // (waves over the channels)
    if (dtype == CB_F16)
        hipLaunchKernelGGL(cbg_detect_kernel<cb_half>, grid, block, 0, (hipStream_t)stream, (const cb_half*)input,
                           (cb_half*)state, (unsigned long long*)frameMasks, words, C, Hi, Wi, Ho, Wo, wprO, *geom,
                           threshold, updateInputState);
    else
        hipLaunchKernelGGL(cbg_detect_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)input,
                           (float*)state, (unsigned long long*)frameMasks, words, C, Hi, Wi, Ho, Wo, wprO, *geom,
                           threshold, updateInputState);
    return cb_launch_status();
}

int cbinfer_conv_changed_geom(const void* input, const int32_t* changeList, int numChanges, const int32_t* countDev,
                              uint64_t* frameMasks, int32_t* idxOut, int32_t* countOut, const void* prepared,
                              const void* bias, void* output, int C, int Hi, int Wi, int K, const cbGeom* geom, int relu,
                              void* workspace, int dtype, cbStream_t stream) {
    CB_REQUIRE(input && prepared && output && C > 0 && K > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16 || dtype == CB_F32S);
    int Ho, Wo;
    const int st = cbg_out_size(Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    if ((long)Ho * Wo >= (1l << 31) / K || (long)C * Hi * Wi * 4 >= (1l << 30)) return CB_ERR_UNSUPPORTED;
    GeomConvParams p = {};
    if (frameMasks) {
        CB_REQUIRE(idxOut && countOut && !changeList);
        p.frameMasks = (unsigned long long*)frameMasks;
        p.maskWords = cbinfer_mask_words(Ho, Wo);
        p.wpr = cbinfer_mask_words_per_row(Wo);
        p.listOut = idxOut, p.countOut = countOut;
    } else {
        CB_REQUIRE(changeList && numChanges >= 0 && numChanges <= Ho * Wo);
        if (numChanges == 0) return CB_OK;
        p.list = changeList, p.countDev = countDev, p.nHost = numChanges;
    }
    const int Ckk = C * geom->kH * geom->kW;
    p.KP = cbg_kpad(K), p.CkkP = cbg_ckkpad(Ckk);
    p.W = prepared;
    p.tab = (const int*)((const char*)prepared + (long)p.KP * p.CkkP * (dtype == CB_F16 ? 2 : 4));
    p.src = input, p.bias = bias, p.out = output;
    if (workspace) {
        p.slabs = (float*)workspace;
        p.tickets = (int*)((char*)workspace + (long)CBG_GRID * CBG_SLAB * 4);
    }
    p.K = K, p.Hi = Hi, p.Wi = Wi, p.Ho = Ho, p.Wo = Wo, p.sH = geom->sH, p.sW = geom->sW, p.relu = relu;
    return cbg_launch_conv(p, dtype, (hipStream_t)stream);
}

int cbinfer_cbconv2d_forward_geom(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                                  int32_t* idx, int32_t* countDev, const void* prepared, const void* bias, int C, int Hi,
                                  int Wi, int K, const cbGeom* geom, float threshold, int feedbackLoop, int copyInput,
                                  int relu, int haveIndexes, int capN, void* workspace, int dtype, cbStream_t stream) {
    CB_REQUIRE(input && prevInput && prevOutput && idx && countDev && prepared);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16 || dtype == CB_F32S);
    int Ho, Wo;
    int st = cbg_out_size(Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    const int edt = dtype == CB_F32S ? CB_F32 : dtype;
    const void* src = (feedbackLoop || copyInput) ? prevInput : input;
    if (haveIndexes) {
        // propagated indexes address the input map: only where it is the output map do they mean what they mean for a
        // unit-geometry layer (no detection ran: the state copy is a copy)
        if (Ho != Hi || Wo != Wi) return CB_ERR_UNSUPPORTED;
        CB_REQUIRE(!feedbackLoop && capN >= 0 && capN <= Ho * Wo);
        if (copyInput && prevInput != input) {
            const hipError_t e = hipMemcpyAsync(prevInput, input, (size_t)C * Hi * Wi * (edt == CB_F16 ? 2 : 4),
                                                hipMemcpyDeviceToDevice, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
        }
        return cbinfer_conv_changed_geom(src, idx, capN, countDev, nullptr, nullptr, nullptr, prepared, bias,
                                         prevOutput, C, Hi, Wi, K, geom, relu, workspace, dtype, stream);
    }
    CB_REQUIRE(frameMasks != nullptr);
    const bool copyAll = !feedbackLoop && copyInput && prevInput != input;
    st = cbinfer_change_detection_geom(input, prevInput, frameMasks, C, Hi, Wi, geom, threshold,
                                       feedbackLoop ? 1 : (copyAll ? 2 : 0), edt, stream);
    if (st != CB_OK) return st;
    return cbinfer_conv_changed_geom(src, nullptr, 0, nullptr, frameMasks, idx, countDev, prepared, bias, prevOutput, C,
                                     Hi, Wi, K, geom, relu, workspace, dtype, stream);
}

}  // extern "C"
