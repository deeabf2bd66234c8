// Change-based deformable convolution (DCNv1 / DCNv2: torchvision.ops.deform_conv2d, mmcv's ModulatedDeformConv2d) on
// gfx950.  The reference has no such operator; the contract and the order of the f32 arithmetic are in
// include/cbinfer_hip.h, which is the specification.  The operator is a grid sampling with a DIFFERENT field per filter
// tap followed by a contraction over C kH kW: a contraction whose pixel operand is SAMPLED, not gathered.  An output pixel
// can differ from last frame's only where its own field values changed or one of its counting taps did, and the offsets
// are data and cannot be inverted, so the frame is driven from the output side as cb_warp.hip's is.  A frame is
//   for an operand in LIST form, one launch in front (cb_list_to_bits): x's list into the working mask of the INPUT map,
//              the field's into the working mask of the OUTPUT map;
//   cbd_foot_kernel      one unit per word of the output mask, a lane per output column: the (offset group, filter tap)
//              pairs are dealt over the four waves, each lane derives its pair's coordinates and tests the change bits of
//              the up to four counting taps in x's mask; the ballots are ORed through LDS with the field's own word and
//              stored as the frame's mask (maskCopy).  A workgroup first ORs x's whole mask -- a few KB -- and skips the
//              tap tests, and with them every field read, when x did not change;
//   cbd_contract_kernel  a persistent grid over tiles of 64 listed pixels x 64 output channels x k-stages of 32 on the
//              MFMA units, the stage images, the MFMA stage, the split along k and the epilogue of cb_geom_stage.h.  The
//              listed pixels are looked up in the frame's mask through a scan of its word counts.  k is TAP-MAJOR (t, c),
//              C padded to 32 per tap: a stage is ONE filter tap and 32 channels, so the four threads that share a pixel
//              need one sample record -- four plane offsets or a not-counting marker, four weights, the multiplier -- for
//              their 8 channels each.  With C / Go a multiple of 8 the record runs one stage ahead of the loads that use
//              it: the x loads of stage s + 1 and the field loads of stage s + 2 are issued before the MFMAs of stage s;
//              any other C / Go builds the record per channel where the group changes (correct, slower);
//   for an x in LIST form, one launch behind: zero to the words of x's working mask that the list named.
// No host sync, memset, allocation or inline assembly of its own; no data atomics beyond the shared split-k ticket.
#include "cb_geom_stage.h"
#include "cb_window.h"

// the sample's arithmetic is specified operation by operation: evaluated as written, never an FMA
#pragma clang fp contract(off)

namespace {

#define CBD_MAXEXT (1 << 15)
#define CBD_LIMIT 1048576.f      // 2^20 px
#define CBD_MAXGROUPS 16

// One axis: s = (float)base + d, clamped (a NaN goes to -L); the bilinear taps i0, i0 + 1 and their weights.
__device__ __forceinline__ void cbd_axis(int base, float d, int& i0, float& w0, float& w1) {
    float s = (float)base + d;
    s = !(s > -CBD_LIMIT) ? -CBD_LIMIT : (s > CBD_LIMIT ? CBD_LIMIT : s);
    const float f = floorf(s);
    i0 = (int)f;
    w0 = (f + 1.f) - s;
    w1 = s - f;
}

// the sample record of one (pixel, offset group, filter tap): element offsets of the taps nw, ne, sw, se in a plane of x
// (-1: the tap does not count; no address is ever formed from it), their weights and the multiplier
struct cbd_rec {
    int o[4];
    float w[4];
    float m;
};

__device__ __forceinline__ void cbd_make_rec(cbd_rec& r, int by, int bx, float dy, float dx, float mraw, int mod, int Hi,
                                             int Wi, bool live) {
    int iy, ix;
    float wy0, wy1, wx0, wx1;
    cbd_axis(by, dy, iy, wy0, wy1);
    cbd_axis(bx, dx, ix, wx0, wx1);
    const bool y0 = live && (unsigned)iy < (unsigned)Hi, y1 = live && (unsigned)(iy + 1) < (unsigned)Hi;
    const bool x0 = (unsigned)ix < (unsigned)Wi, x1 = (unsigned)(ix + 1) < (unsigned)Wi;
    r.o[0] = (y0 && x0) ? iy * Wi + ix : -1;
    r.o[1] = (y0 && x1) ? iy * Wi + ix + 1 : -1;
    r.o[2] = (y1 && x0) ? (iy + 1) * Wi + ix : -1;
    r.o[3] = (y1 && x1) ? (iy + 1) * Wi + ix + 1 : -1;
    r.w[0] = wx0 * wy0;
    r.w[1] = wx1 * wy0;
    r.w[2] = wx0 * wy1;
    r.w[3] = wx1 * wy1;
    r.m = mod == CB_DEFORM_SIGMOID ? 1.f / (1.f + expf(-mraw)) : mraw;
}

// the modulated sample from the four tap values (+0 was loaded for a tap that does not count, and is not used)
__device__ __forceinline__ float cbd_sample(const cbd_rec& r, const float (&p)[4], int mod) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float term = r.w[k] * p[k];
        acc = r.o[k] >= 0 ? acc + term : acc;
    }
    if (mod != CB_DEFORM_NONE) acc = acc * r.m;
    return acc;
}

// ---------------------------------------------------------------------------------------------
// weight preparation: W[K][C][T] -> Wp[KP][T][Cp] in the tensors' element type, zero padded (Cp: C padded to 32)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cbd_prep_kernel(const T* __restrict__ w, T* __restrict__ wp, int K, int C, int taps,
                                                      int Cp, long total) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int CkkP = taps * Cp;
    const int k = (int)(e % CkkP), m = (int)(e / CkkP);
    const int t = k / Cp, c = k - t * Cp;
    wp[e] = (m < K && c < C) ? w[((long)m * C + c) * taps + t] : T(0);
}

// ---------------------------------------------------------------------------------------------
// launch 1: the frame's mask.  xMask: x's change mask of this frame over the INPUT map (its own, or the working mask its
// list went into), or NULL: x did not change; fMask: the field's over the output map, or NULL (a list is in `bits`
// already); all: every output pixel is listed, neither mask is read.
// ---------------------------------------------------------------------------------------------
template <typename FT>
__global__ __launch_bounds__(256) void cbd_foot_kernel(const FT* __restrict__ field,
                                                      const unsigned long long* __restrict__ xMask, long xWords,
                                                      const unsigned long long* __restrict__ fMask, int all,
                                                      unsigned long long* bits, unsigned long long* __restrict__ maskCopy,
                                                      long words, int Go, int Hi, int Wi, int Ho, int Wo, int wprI,
                                                      int wprO, cbGeom g) {
    // the four waves' ballots, used in turn: a region is written again only behind the barrier of the word after it
    __shared__ unsigned long long foot[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long HWo = (long)Ho * Wo;
    const int taps = g.kH * g.kW, pairs = Go * taps;
    int anyX = 0;
    if (!all && xMask) {      // (uniform over the workgroup)
        unsigned long long a = 0ull;
        for (long w = threadIdx.x; w < xWords; w += 256) a |= xMask[w];
        anyX = __syncthreads_or(a != 0ull);
    }
    unsigned turn = 0;
    cb_walk_word_units(
        bits, maskCopy, words, Wo, wprO, all,
        [&](long w, int oy, int tile) {
            if (all) return 0ull;
            unsigned long long word = fMask ? fMask[w] : 0ull;
            if (anyX) {
                const int ox = tile * 64 + lane;
                bool hit = false;
                if (ox < Wo) {
                    const FT* f = field + (long)oy * Wo + ox;
                    for (int e = wave; e < pairs && !hit; e += 4) {      // wave v tests the pairs v, v + 4, ...
                        const int t = e % taps, ky = t / g.kW, kx = t - ky * g.kW;
                        int iy, ix;
                        float w0, w1;
                        cbd_axis(oy * g.sH - g.pH + ky * g.dH, cb_load_f32(f + (long)(2 * e) * HWo), iy, w0, w1);
                        cbd_axis(ox * g.sW - g.pW + kx * g.dW, cb_load_f32(f + (long)(2 * e + 1) * HWo), ix, w0, w1);
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if ((unsigned)(iy + j) >= (unsigned)Hi) continue;
                            const unsigned long long* row = xMask + (long)(iy + j) * wprI;
#pragma unroll
                            for (int i = 0; i < 2; ++i) {
                                const int xx = ix + i;
                                if ((unsigned)xx < (unsigned)Wi) hit |= ((row[xx >> 6] >> (xx & 63)) & 1ull) != 0;
                            }
                        }
                    }
                }
                const unsigned long long mine = __ballot(hit);
                unsigned long long* fo = foot[turn++ & 1u];
                if (lane == 0) fo[wave] = mine;
                __syncthreads();
                word |= fo[0] | fo[1] | fo[2] | fo[3];
            }
            return word;
        },
        [&](unsigned long long, int, int) {});
}

// ---------------------------------------------------------------------------------------------
// launch 2: the sampled contraction
// ---------------------------------------------------------------------------------------------
struct DeformParams {
    const void* W;         // prepared weights [KP][T][Cp]
    const void* x;         // [C, Hi, Wi]
    const void* field;     // [F, Ho, Wo]
    const void* bias;      // [K] or null
    void* out;             // [K, Ho, Wo]
    const unsigned long long* mask;      // the frame's mask (launch 1 left it in maskCopy)
    long words;
    int wpr;
    CbgWorkspace ws;
    int C, Cg, Cp, taps, Go, K, KP, CkkP, Hi, Wi, Ho, Wo, mod, relu;
    cbGeom g;
};

// T, ARITH: the tensors' element type and the arithmetic (CB_F16; CB_F32S for float); FT: the field's element type;
// RUN8: C / Go is a multiple of 8 -- a thread's 8 channels of a stage lie in one offset group.
template <typename T, typename FT, int ARITH, bool RUN8>
__global__ __launch_bounds__(256) void cbd_contract_kernel(DeformParams p) {
    __shared__ CbgStage<ARITH> sA[2], sB[2];
    __shared__ int sPre[257];
    __shared__ int sList[CBG_BN];
    __shared__ int sLast;
    __shared__ int sWave[4];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int G = gridDim.x, HWo = p.Ho * p.Wo, HWi = p.Hi * p.Wi;

    // ---- the listed pixels: every workgroup scans the word counts of the frame's mask (thread t the words
    // [t chunk, (t + 1) chunk), the layout cbg_list_entry looks an entry up in); nothing is written
    const unsigned long long* cur = p.mask;
    const long words = p.words;
    const int chunk = (int)((words + 255) / 256);
    {
        const long w0 = (long)t * chunk, w1 = min(words, w0 + chunk);
        int inc = 0;
        for (long w = w0; w < w1; ++w) inc += __popcll(cur[w]);
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
    }
    const int N = sPre[256];
    if (N == 0) return;

    // ---- work items: (pixel tile, channel tile, k-slice), as cbg_conv_kernel's
    const int tilesN = (N + CBG_BN - 1) / CBG_BN, tilesM = p.KP / CBG_BM, stages = p.CkkP / CBG_BK;
    const int spt = p.Cp / CBG_BK;      // stages per filter tap
    const int base = tilesN * tilesM;
    int SK = 1;
    if (base < G) SK = max(1, min(min(G / base, CBG_SKMAX), stages));
    const int items = base * SK;      // (SK > 1: items <= G, one item and one slab per workgroup)
    const int gn = t & 63, gk = wave * 8;      // the thread's place in the tile (cb_geom_stage.h)
    const int am = t >> 2, ak = (t & 3) * 8;
    const int wm = wave & 1, wn = wave >> 1;
    const T* src = (const T*)p.x;
    const FT* field = (const FT*)p.field;
    const int mod = p.mod;

    for (int item = blockIdx.x; item < items; item += G) {
        const int slice = item % SK, tm = (item / SK) % tilesM, tn = item / (SK * tilesM);
        const int s0 = (int)((long)stages * slice / SK), s1 = (int)((long)stages * (slice + 1) / SK);
        __syncthreads();
        if (t < CBG_BN) {
            const int q = tn * CBG_BN + t;
            sList[t] = q < N ? cbg_list_entry(q, cur, sPre, words, chunk, p.wpr, p.Wo, nullptr, HWo) : -1;
        }
        __syncthreads();

        const int pix = sList[gn];
        const int oy = pix < 0 ? 0 : pix / p.Wo, ox = pix < 0 ? 0 : pix - (pix / p.Wo) * p.Wo;
        const int by0 = oy * p.g.sH - p.g.pH, bx0 = ox * p.g.sW - p.g.pW;
        const FT* fpix = field + (pix < 0 ? 0 : pix);
        const T* wrow = (const T*)p.W + ((long)tm * CBG_BM + am) * p.CkkP + ak;

        // stage s is filter tap s / spt and the channels (s % spt) 32 ..; this thread's 8 start at c0
        // the raw field values of (group gI, tap tap) at this thread's pixel; nothing is read for a dead row
        auto fieldLoad = [&](int gI, int tap, bool live, float& fdy, float& fdx, float& fm) {
            fdy = fdx = fm = 0.f;
            if (live) {
                const long e = (long)gI * p.taps + tap;
                fdy = cb_load_f32(fpix + 2 * e * HWo);
                fdx = cb_load_f32(fpix + (2 * e + 1) * HWo);
                if (mod != CB_DEFORM_NONE) fm = cb_load_f32(fpix + (2l * p.Go * p.taps + e) * HWo);
            }
        };
        auto makeRec = [&](cbd_rec& r, int tap, bool live, float fdy, float fdx, float fm) {
            const int ky = tap / p.g.kW, kx = tap - ky * p.g.kW;
            cbd_make_rec(r, by0 + ky * p.g.dH, bx0 + kx * p.g.dW, fdy, fdx, fm, mod, p.Hi, p.Wi, live);
        };
        // the four tap values of channel c (< C) through record r
        auto tapLoad = [&](const cbd_rec& r, int c, float (&v)[4]) {
            const T* plane = src + c * HWi;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = r.o[k] >= 0 ? cb_load_f32(plane + r.o[k]) : 0.f;
        };

        T ra[8], rb[8];
        floatx16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;

        if constexpr (RUN8) {
            // the record runs one stage ahead of the loads that use it, the field loads two
            cbd_rec rec;
            float raw[8][4], fdy, fdx, fm;
            bool liveN = false;      // the field values in flight belong to a live (pixel, channel run)
            auto place = [&](int s, int& tap, int& c0) {
                tap = s / spt;
                c0 = (s - tap * spt) * CBG_BK + gk;
            };
            auto issueField = [&](int s) {
                int tap, c0;
                place(s, tap, c0);
                liveN = pix >= 0 && c0 < p.C;
                fieldLoad(liveN ? c0 / p.Cg : 0, tap, liveN, fdy, fdx, fm);
            };
            auto finishRec = [&](int s) {
                int tap, c0;
                place(s, tap, c0);
                makeRec(rec, tap, liveN, fdy, fdx, fm);
            };
            auto issueX = [&](int s) {
                int tap, c0;
                place(s, tap, c0);
                cbg_load_wrow(ra, wrow + (long)s * CBG_BK);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (c0 + i < p.C) {
                        tapLoad(rec, c0 + i, raw[i]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) raw[i][k] = 0.f;
                    }
                }
            };
            auto finishX = [&]() {
#pragma unroll
                for (int i = 0; i < 8; ++i) rb[i] = (T)cbd_sample(rec, raw[i], mod);
            };
            if (s0 < s1) {
                issueField(s0);
                finishRec(s0);
                issueX(s0);
                if (s0 + 1 < s1) issueField(s0 + 1);
                finishX();
                sA[0].put(am, ak, ra);
                sB[0].put(gn, gk, rb);
                if (s0 + 1 < s1) finishRec(s0 + 1);
            }
            __syncthreads();
            for (int s = s0; s < s1; ++s) {
                const int cb = (s - s0) & 1;
                if (s + 1 < s1) issueX(s + 1);
                if (s + 2 < s1) issueField(s + 2);
                acc = cbg_mfma_stage<ARITH>(sA[cb], sB[cb], wm * 32 + (lane & 31), wn * 32 + (lane & 31), lane, acc);
                if (s + 1 < s1) {
                    finishX();
                    sA[cb ^ 1].put(am, ak, ra);
                    sB[cb ^ 1].put(gn, gk, rb);
                }
                if (s + 2 < s1) finishRec(s + 2);
                __syncthreads();
            }
        } else {
            // any C / Go: the record is rebuilt where a channel enters another offset group
            auto load = [&](int s) {
                const int tap = s / spt, c0 = (s - tap * spt) * CBG_BK + gk;
                cbg_load_wrow(ra, wrow + (long)s * CBG_BK);
                cbd_rec rec;
                int gHave = -1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int c = c0 + i;
                    float v[4] = {0.f, 0.f, 0.f, 0.f};
                    float val = 0.f;
                    if (pix >= 0 && c < p.C) {
                        const int gI = c / p.Cg;
                        if (gI != gHave) {
                            float fdy, fdx, fm;
                            fieldLoad(gI, tap, true, fdy, fdx, fm);
                            makeRec(rec, tap, true, fdy, fdx, fm);
                            gHave = gI;
                        }
                        tapLoad(rec, c, v);
                        val = cbd_sample(rec, v, mod);
                    }
                    rb[i] = (T)val;
                }
            };
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
        }
        if (SK > 1) CBG_SPLITK_HANDOFF(acc, p.ws.slabs, p.ws.tickets + (tn * tilesM + tm), item, slice, SK, sLast, continue)
        CBG_TILE_STORE(acc, sList, tm, p.bias, p.out, p.K, HWo, p.relu)
    }
}

inline bool cbd_extent_ok(int n) { return n >= 1 && n < CBD_MAXEXT; }
inline int cbd_cpad(int C) { return (C + CBG_BK - 1) / CBG_BK * CBG_BK; }

template <typename T, typename FT, int ARITH>
void cbd_launch_contract(const DeformParams& p, hipStream_t s) {
    if (p.Cg % 8 == 0)
        hipLaunchKernelGGL((cbd_contract_kernel<T, FT, ARITH, true>), dim3(CBG_GRID), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((cbd_contract_kernel<T, FT, ARITH, false>), dim3(CBG_GRID), dim3(256), 0, s, p);
}

}  // namespace

extern "C" {

int cbinfer_deform_supported(const cbDeform* d, int C, int Hi, int Wi, int K) {
    if (!d || C < 1 || K < 1 || !cbd_extent_ok(Hi) || !cbd_extent_ok(Wi)) return 0;
    int Ho = 0, Wo = 0;
    if (cbinfer_geom_out_size(Hi, Wi, &d->geom, &Ho, &Wo) != CB_OK) return 0;
    if (!cbd_extent_ok(Ho) || !cbd_extent_ok(Wo)) return 0;
    if (d->offsetGroups < 1 || d->offsetGroups > CBD_MAXGROUPS || C % d->offsetGroups) return 0;
    if (d->modulation < CB_DEFORM_NONE || d->modulation > CB_DEFORM_SIGMOID) return 0;
    if ((d->fieldDtype != CB_F32 && d->fieldDtype != CB_F16) || (d->relu != 0 && d->relu != 1)) return 0;
    // tap offsets and output offsets are ints; the k extent and the channel tiles are ints with room to spare
    if ((long)C * Hi * Wi * 4 >= (1l << 30) || (long)Ho * Wo >= (1l << 31) / K) return 0;
    if ((long)d->geom.kH * d->geom.kW * cbd_cpad(C) >= (1l << 24) || K >= (1 << 20)) return 0;
    return 1;
}

long cbinfer_deform_prepared_weights_bytes(int K, int C, const cbDeform* d, int dtype) {
    if (!d || K < 1 || C < 1 || K >= (1 << 20) || (dtype != CB_F32 && dtype != CB_F16)) return 0;
    int Ho, Wo;      // (a geometry within the limits fits a map that large)
    if (cbinfer_geom_out_size(1024, 1024, &d->geom, &Ho, &Wo) != CB_OK) return 0;
    const long CkkP = (long)d->geom.kH * d->geom.kW * cbd_cpad(C);
    if (CkkP >= (1l << 24)) return 0;
    return (long)cbg_kpad(K) * CkkP * (dtype == CB_F16 ? 2 : 4);
}

int cbinfer_deform_prep_weights(const void* weight, void* prepared, int K, int C, const cbDeform* d, int dtype,
                                cbStream_t stream) {
    CB_REQUIRE(weight && prepared && d);
    const long bytes = cbinfer_deform_prepared_weights_bytes(K, C, d, dtype);
    CB_REQUIRE(bytes > 0);
    const int taps = d->geom.kH * d->geom.kW, Cp = cbd_cpad(C);
    const long total = bytes / (dtype == CB_F16 ? 2 : 4);
    dim3 grid(cb_div_up(total, 256)), block(256);
    if (dtype == CB_F16)
        hipLaunchKernelGGL(cbd_prep_kernel<cb_half>, grid, block, 0, (hipStream_t)stream, (const cb_half*)weight,
                           (cb_half*)prepared, K, C, taps, Cp, total);
    else
        hipLaunchKernelGGL(cbd_prep_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)weight,
                           (float*)prepared, K, C, taps, Cp, total);
    return cb_launch_status();
}

int cbinfer_cbdeform_forward(const void* x, const void* field, const void* preparedW, const void* bias, void* outputState,
                             const uint64_t* maskX, const int32_t* listX, int capX, const int32_t* countX,
                             const uint64_t* maskF, const int32_t* listF, int capF, const int32_t* countF,
                             uint64_t* inBits, uint64_t* bits, uint64_t* maskCopy, void* workspace, int C, int Hi, int Wi,
                             int K, const cbDeform* deform, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(x && field && preparedW && workspace && outputState && outputState != x && outputState != field);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_deform_supported(deform, C, Hi, Wi, K));
    // (cb_window.h's operand A is read at the pixel itself: the field; its operand B at the taps: x)
    const cbw_forms f = {maskF, listF, capF, countF, maskX, listX, capX, countX, inBits, bits, maskCopy};
    CB_REQUIRE(cbw_forms_ok(f));
    int Ho, Wo;
    CB_REQUIRE(cbinfer_geom_out_size(Hi, Wi, &deform->geom, &Ho, &Wo) == CB_OK);
    const hipStream_t s = (hipStream_t)stream;
    // an operand with neither mask nor list lists every output pixel: the other's changes are not needed then
    const int all = (!maskX && !listX) || (!maskF && !listF);
    const bool xList = !all && listX && capX > 0;
    if (xList) {
        const int st = cb_list_to_bits(listX, capX, countX, Hi, Wi, inBits, stream);
        if (st != CB_OK) return st;
    }
    if (!all && listF) {
        const int st = cb_list_to_bits(listF, capF, countF, Ho, Wo, bits, stream);
        if (st != CB_OK) return st;
    }
    const uint64_t* xMask = all ? nullptr : (maskX ? maskX : (xList ? inBits : nullptr));
    const int wprI = cbinfer_mask_words_per_row(Wi), wprO = cbinfer_mask_words_per_row(Wo);
    const long words = (long)Ho * wprO, xWords = (long)Hi * wprI;
    cb_dispatch_dtype(deform->fieldDtype, [&](auto ft) {
        typedef decltype(ft) FT;
        hipLaunchKernelGGL(cbd_foot_kernel<FT>, dim3(cb_walk_grid(words)), dim3(256), 0, s, (const FT*)field,
                           (const unsigned long long*)xMask, xWords, (const unsigned long long*)(all ? nullptr : maskF),
                           all, (unsigned long long*)bits, (unsigned long long*)maskCopy, words, deform->offsetGroups, Hi,
                           Wi, Ho, Wo, wprI, wprO, deform->geom);
    });
    int st = cb_launch_status();
    if (st != CB_OK) return st;

    DeformParams p = {};
    p.W = preparedW, p.x = x, p.field = field, p.bias = bias, p.out = outputState;
    p.mask = (const unsigned long long*)maskCopy, p.words = words, p.wpr = wprO;
    p.ws = cbg_workspace(workspace);
    p.C = C, p.Go = deform->offsetGroups, p.Cg = C / p.Go, p.Cp = cbd_cpad(C);
    p.taps = deform->geom.kH * deform->geom.kW;
    p.K = K, p.KP = cbg_kpad(K), p.CkkP = p.taps * p.Cp;
    p.Hi = Hi, p.Wi = Wi, p.Ho = Ho, p.Wo = Wo, p.mod = deform->modulation, p.relu = deform->relu, p.g = deform->geom;
    cb_dispatch_dtype(deform->fieldDtype, [&](auto ft) {
        typedef decltype(ft) FT;
        if (dtype == CB_F16)
            cbd_launch_contract<cb_half, FT, CB_F16>(p, s);
        else
            cbd_launch_contract<float, FT, CB_F32S>(p, s);
    });
    st = cb_launch_status();
    if (st != CB_OK || !xList) return st;
    return cbw_clear_list(f, Hi, Wi, s);
}

}  // extern "C"
