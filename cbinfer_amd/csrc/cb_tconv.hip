// Change-based transposed convolution for gfx950 (nn.ConvTranspose2d: the learned upsampling of U-Net, segmentation and
// depth decoders, DCGAN-type generators).
//   input map  Hi x Wi, weight [C, K, kH, kW], stride (sH, sW), padding (pH, pW), dilation (dH, dW), output padding
//   output map Ho = (Hi - 1) sH - 2 pH + dH (kH - 1) + opH + 1, Wo likewise
//   out[co, oy, ox] = bias[co] + sum over c and the taps (ky, kx) with  ny = oy + pH - ky dH = sH iy,
//                     nx = ox + pW - kx dW = sW ix,  (iy, ix) inside the input map,  of  in[c, iy, ix] w[c, co, ky, kx]
// The stride makes sH sW classes of output pixels (PHASES, ((oy + pH) mod sH, (ox + pW) mod sW)), and each phase reads
// its own subset of the filter taps -- tap ky belongs to row phase ry iff (ry - ky dH) mod sH == 0 --, possibly none.
// A tile of listed pixels can share one weight matrix only if its pixels have one phase: the contraction's tiles are
// phase-homogeneous and every phase has its own compact k axis of C taps(phase) entries.  Two launches per frame:
//   cbt_detect_kernel  per-pixel change on the INPUT map (component a1's rule), state refresh, and the exact footprint
//                      of the changed pixels ORed into a row-padded bit mask of the OUTPUT map (frame-mask protocol:
//                      two alternating masks + parity, cbinfer_frame_mask_bytes);
//   cbt_conv_kernel    counts the listed pixels per phase from that mask (or from a caller's list) by itself, gathers
//                      the taps of 64 listed pixels of ONE phase per tile through that phase's k -> tap table and
//                      contracts them with that phase's weight matrix: the stages, the MFMA forms, the split along k
//                      and the epilogue are the shared 64 x 64 x 32 tile's (cb_geom_stage.h: CBG_TILE_STAGES,
//                      CBG_SPLITK_HANDOFF, CBG_TILE_STORE), as in cbg_conv_kernel.
// Entry-point contracts: include/cbinfer_hip.h, "transposed convolution".
#include "cb_common.h"
#include "cb_geom_stage.h"

namespace {

#define CBT_MAX_K 8      // filter size per axis
#define CBT_MAX_S 4      // stride per axis
#define CBT_MAX_D 4      // dilation per axis
#define CBT_MAX_PH 16    // phases

int cbt_geom_status(const cbTGeom* g) {
    if (!g) return CB_ERR_BADARG;
    if (g->kH < 1 || g->kW < 1 || g->sH < 1 || g->sW < 1 || g->dH < 1 || g->dW < 1 || g->pH < 0 || g->pW < 0 ||
        g->opH < 0 || g->opW < 0)
        return CB_ERR_BADARG;
    if (g->kH > CBT_MAX_K || g->kW > CBT_MAX_K || g->sH > CBT_MAX_S || g->sW > CBT_MAX_S || g->dH > CBT_MAX_D ||
        g->dW > CBT_MAX_D || g->pH > g->dH * (g->kH - 1) || g->pW > g->dW * (g->kW - 1) ||
        g->opH >= (g->sH > g->dH ? g->sH : g->dH) || g->opW >= (g->sW > g->dW ? g->sW : g->dW))
        return CB_ERR_UNSUPPORTED;
    return CB_OK;
}

int cbt_out_size(int Hi, int Wi, const cbTGeom* g, long* Ho, long* Wo) {
    const int st = cbt_geom_status(g);
    if (st != CB_OK) return st;
    if (Hi < 1 || Wi < 1) return CB_ERR_BADARG;
    *Ho = (long)(Hi - 1) * g->sH - 2 * g->pH + g->dH * (g->kH - 1) + g->opH + 1;
    *Wo = (long)(Wi - 1) * g->sW - 2 * g->pW + g->dW * (g->kW - 1) + g->opW + 1;
    if (*Ho < 1 || *Wo < 1) return CB_ERR_BADARG;      // (the padding eats the whole output of a map this small)
    return CB_OK;
}

// the taps of one axis that belong to phase r: their number, and the n-th of them (ascending)
__host__ __device__ inline int cbt_ntaps(int k, int d, int s, int r) {
    int n = 0;
    for (int i = 0; i < k; ++i) n += (i * d - r) % s == 0;
    return n;
}
__host__ __device__ inline int cbt_nth_tap(int k, int d, int s, int r, int n) {
    for (int i = 0; i < k; ++i)
        if ((i * d - r) % s == 0 && n-- == 0) return i;
    return 0;
}

// per phase ph = ry sW + rx: padded k-depth (0: the phase owns no tap) and byte offset of its weight matrix
// W_ph[KP][ckkP] (followed by its tap table, 2 ckkP ints) in the prepared buffer
struct TConvLayout {
    int ckkP[CBT_MAX_PH];
    long wOff[CBT_MAX_PH];
    long total;
};

TConvLayout cbt_layout(int K, int C, const cbTGeom* g, int dtype) {
    TConvLayout L = {};
    const long KP = cbg_kpad(K), es = dtype == CB_F16 ? 2 : 4;
    for (int ry = 0; ry < g->sH; ++ry)
        for (int rx = 0; rx < g->sW; ++rx) {
            const int ph = ry * g->sW + rx;
            const long ckk = (long)C * cbt_ntaps(g->kH, g->dH, g->sH, ry) * cbt_ntaps(g->kW, g->dW, g->sW, rx);
            const long ckkP = (ckk + CBG_BK - 1) / CBG_BK * CBG_BK;
            L.ckkP[ph] = (int)ckkP;
            L.wOff[ph] = L.total;
            L.total += KP * ckkP * es + ckkP * 8;
        }
    return L;
}

// shape checks shared by the entry points: CB_OK and the output size, or the status
int cbt_shape(int C, int K, int Hi, int Wi, const cbTGeom* g, int* Ho, int* Wo) {
    long ho, wo;
    const int st = cbt_out_size(Hi, Wi, g, &ho, &wo);
    if (st != CB_OK) return st;
    if (C < 1 || K < 1) return CB_ERR_BADARG;
    const long lim = 0x7fffffffl;
    if (ho * wo > lim || (long)C * Hi * Wi > lim || ho * wo > lim / K) return CB_ERR_BADARG;
    if ((long)C * Hi * Wi * 4 >= (1l << 30)) return CB_ERR_UNSUPPORTED;      // (tap offsets are 32-bit byte offsets)
    *Ho = (int)ho, *Wo = (int)wo;
    return CB_OK;
}

// ---------------------------------------------------------------------------------------------
// weight preparation, blockIdx.y = phase: W_ph[KP][ckkP] in the tensors' element type (k = c taps + tap, contiguous,
// zero padded) from torch's [C, K, kH, kW], then the phase's k -> tap table.  An output pixel (oy, ox) of phase
// (ry, rx) has oy + pH = sH iy0 + ry: (iy0, ix0) is its BASE input pixel, and tap (ky, kx) reads (iy0 + dy, ix0 + dx),
// dy = (ry - ky dH) / sH, dx = (rx - kx dW) / sW (exact divisions); the table entry is cbg_tab_entry's
// (cb_geom_stage.h), whose marker for the padded tail is outside every map cbt_shape admits.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cbt_prep_kernel(const T* __restrict__ w, char* __restrict__ prepared, int K, int C,
                                                      int KP, int Hi, int Wi, cbTGeom g, TConvLayout L) {
    const int ph = blockIdx.y, CkkP = L.ckkP[ph];
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)KP * CkkP) return;
    const int ry = ph / g.sW, rx = ph % g.sW;
    const int ntW = cbt_ntaps(g.kW, g.dW, g.sW, rx), nt = cbt_ntaps(g.kH, g.dH, g.sH, ry) * ntW, Ckk = C * nt;
    T* wp = (T*)(prepared + L.wOff[ph]);
    const int k = (int)(e % CkkP), m = (int)(e / CkkP);
    int c = 0, ky = 0, kx = 0;
    if (k < Ckk) {
        c = k / nt;
        ky = cbt_nth_tap(g.kH, g.dH, g.sH, ry, (k % nt) / ntW);
        kx = cbt_nth_tap(g.kW, g.dW, g.sW, rx, (k % nt) % ntW);
    }
    if (m == 0)
        cbg_tab_entry<T>((int*)(wp + (long)KP * CkkP), CkkP, k, k >= Ckk, c, (ry - ky * g.dH) / g.sH,
                         (rx - kx * g.dW) / g.sW, Hi, Wi);
    wp[e] = (m < K && k < Ckk) ? w[(((long)c * K + m) * g.kH + ky) * g.kW + kx] : T(0);
}

// x mod s and x / s for x >= 0 and a stride 1 <= s <= 4 without the integer-division sequence (some forty instructions
// for a divisor the compiler does not know; these run per mask word and per list entry at the head of every launch)
__device__ __forceinline__ int cbt_mod_s(int x, int s) { return s == 1 ? 0 : s == 2 ? (x & 1) : s == 4 ? (x & 3) : x % 3; }
__device__ __forceinline__ int cbt_div_s(int x, int s) { return s == 1 ? x : s == 2 ? (x >> 1) : s == 4 ? (x >> 2) : x / 3; }

// ---------------------------------------------------------------------------------------------
// detection: cbg_detect_kernel's form -- one workgroup = one 64-pixel row segment of the INPUT map x all channels (1 to
// 16 waves); the scan and the state refresh are cbg_detect_scan (cb_geom_stage.h).
// The footprint in gather form on wave 0: for every output word the segment can reach (columns x0 sW - pW ..
// (x0 + 63) sW - pW + (kW-1) dW: up to six words with s = 4, k = 8, d = 4), lane j owns output column ox = 64 w + j and
// tests the input bits of its column-valid taps (nx = ox + pW - kx dW >= 0, divisible by sW, nx / sW in the segment);
// a ballot makes the word, which is ORed into the output rows oy = y sH - pH + ky dH that lie inside the map (lane ky;
// distinct ky give distinct rows).  A changed pixel that reaches no output pixel still refreshes the state.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void cbt_detect_kernel(const T* __restrict__ in, T* state,
                                                        unsigned long long* __restrict__ masks, long maskWords, int C,
                                                        int Hi, int Wi, int Ho, int Wo, int wprO, cbTGeom g, float thf,
                                                        int update) {
    unsigned long long* bits = masks;
    if (*(const int*)(masks + 2 * maskWords)) bits += maskWords;      // the mask the parity selects
    const int lane = threadIdx.x & 63, tx = blockIdx.x, y = blockIdx.y;
    const int x = tx * 64 + lane;
    const unsigned long long m = cbg_detect_scan(in, state, C, (long)Hi * Wi, (long)y * Wi + x, x < Wi, thf, update);
    if (m == 0) return;      // uniform over the workgroup
    if (threadIdx.x >> 6 != 0) return;      // (the footprint: wave 0)

    const int x0 = tx * 64;
    const int oxLo = max(0, x0 * g.sW - g.pW);
    const int oxHi = min((x0 + 63) * g.sW - g.pW + (g.kW - 1) * g.dW, Wo - 1);
    if (oxLo > oxHi) return;
    // lane r < kH: the output row this input row feeds through filter row r
    const int oy = y * g.sH - g.pH + lane * g.dH;
    const bool rowOk = lane < g.kH && oy >= 0 && oy < Ho;
    for (int w = oxLo >> 6; w <= (oxHi >> 6); ++w) {
        const int ox = w * 64 + lane;
        bool bit = false;
        if (ox < Wo)
            for (int kx = 0; kx < g.kW; ++kx) {
                const int nx = ox + g.pW - kx * g.dW;
                const int bpos = cbt_div_s(nx, g.sW) - x0;
                if (nx >= 0 && cbt_mod_s(nx, g.sW) == 0 && (unsigned)bpos < 64u) bit |= (m >> bpos) & 1ull;
            }
        const unsigned long long word = __ballot(bit);
        if (word && rowOk) atomicOr(&bits[(long)oy * wprO + w], word);
    }
}

// ---------------------------------------------------------------------------------------------
// contraction
// ---------------------------------------------------------------------------------------------
struct TConvParams {
    const char* prepared;    // per phase: W_ph[KP][ckkP], tap table
    const void* src;         // the map the gather reads [C, Hi, Wi]
    const void* bias;        // [K] or null
    void* out;               // [K, Ho, Wo]
    CbgListArgs L;
    CbgWorkspace ws;
    int K, KP, Hi, Wi, Ho, Wo, sH, sW, pH, pW, relu;
    double rWo;                        // 1 / Wo
    int ckkP[CBT_MAX_PH];
    long wOff[CBT_MAX_PH];
};

// the bits of the mask word at row yy, word column col (pixels 64 col ..) whose pixels have phase (ry, rx): the row
// phase is fixed per word, the column phases are sW fixed bit patterns shifted by the word's first column
__device__ __forceinline__ unsigned long long cbt_phase_bits(const TConvParams& p, int ry, int rx, int yy, int col) {
    if (cbt_mod_s(yy + p.pH, p.sH) != ry) return 0ull;
    const unsigned long long every = p.sW == 1   ? ~0ull
                                     : p.sW == 2 ? 0x5555555555555555ull
                                     : p.sW == 3 ? 0x9249249249249249ull
                                                 : 0x1111111111111111ull;      // (bits j with j % sW == 0)
    const int r = rx - cbt_mod_s(col * 64 + p.pW, p.sW);
    return every << (r < 0 ? r + p.sW : r);
}
// row and column of flat output pixel pix, 0 <= pix < Ho Wo < 2^31 (the quotient through the reciprocal, one step off at
// the most)
__device__ __forceinline__ void cbt_row_col(const TConvParams& p, int pix, int& oy, int& ox) {
    oy = (int)((double)pix * p.rWo);
    ox = pix - oy * p.Wo;
    if (ox < 0) ox += p.Wo, --oy;
    if (ox >= p.Wo) ox -= p.Wo, ++oy;
}
// the phase of flat output pixel pix, -1 outside the map
__device__ __forceinline__ int cbt_phase_of(const TConvParams& p, int pix) {
    if (pix < 0 || pix >= p.Ho * p.Wo) return -1;
    int oy, ox;
    cbt_row_col(p, pix, oy, ox);
    return cbt_mod_s(oy + p.pH, p.sH) * p.sW + cbt_mod_s(ox + p.pW, p.sW);
}

// T, ARITH, the 2 x 2 waves, the stage pipeline, the split along k and the epilogue: the shared tile of cb_geom_stage.h
// (CBG_TILE_STAGES, CBG_SPLITK_HANDOFF, CBG_TILE_STORE).  This kernel's own: work items are (phase, pixel tile of that
// phase, channel tile, k-slice), and the base input pixel is ((oy + pH) / sH, (ox + pW) / sW).  The listed pixels of a
// phase are found through ONE prefix table over 256 chunks (of mask words, or of list entries), built for the phase of
// the item at hand: every thread keeps its chunk's count per phase in registers (one pass at launch start, which also gives the
// totals per phase, sTot), and the table is a scan of those -- built for the first item and again only when a
// workgroup's next item has another phase, never while base <= grid, where a workgroup has one item.  LDS: the F32S
// stage buffers leave 2.7 KB under the 64 KB static limit, which per-phase tables (16 x 257 ints) would exceed.
template <typename T, int ARITH>
__global__ __launch_bounds__(256) void cbt_conv_kernel(TConvParams p) {
    __shared__ CbgStage<ARITH> sA[2], sB[2];
    __shared__ int sPre[257];
    __shared__ int sList[CBG_BN];
    __shared__ int sTot[CBT_MAX_PH];
    __shared__ int sLast;
    __shared__ int sWave[4];
    __shared__ int sWaveTot[4][CBT_MAX_PH];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int G = CBG_GRID, HWo = p.Ho * p.Wo, P = p.sH * p.sW;      // (the launcher's grid)

    const unsigned long long* cur = nullptr;
    const int words = (int)p.L.maskWords;      // (Ho Wo < 2^31)
    int par = 0, nList = 0;
    if (p.L.frameMasks) {
        par = __hip_atomic_load((int*)(p.L.frameMasks + 2 * words), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cur = p.L.frameMasks + (par ? words : 0);
    } else {
        nList = CBG_LIST_COUNT(p.L, HWo);
    }
    // thread t's chunk: of the mask's words, or of the list's entries
    const int total = cur ? words : nList;
    const int chunk = (total + 255) / 256;
    const int c0 = (int)min((long)total, (long)t * chunk), c1 = min(total, c0 + chunk);
    const int y0 = cur ? c0 / p.L.wpr : 0, col0 = cur ? c0 - y0 * p.L.wpr : 0;      // (the chunk's first word)

    // ONE pass over the chunk, four loads in flight (a dependent load per element and phase was most of a short
    // launch): per phase this thread's number of listed pixels.  The phase loops are unrolled, so the array is never
    // indexed by a variable and stays in registers -- for the prefix table of every item this workgroup walks.  The
    // same pass writes the mask copy and the zeros of the OTHER mask (the next frame's) for the workgroup's share of
    // the words.
    int cnt[CBT_MAX_PH];
#pragma unroll
    for (int i = 0; i < CBT_MAX_PH; ++i) cnt[i] = 0;
    if (cur) {
        unsigned long long* other = p.L.frameMasks + (par ? 0 : words);
        unsigned long long* copy = p.L.frameMasks + 2 * words + 2;
        const unsigned long long every = p.sW == 1   ? ~0ull
                                         : p.sW == 2 ? 0x5555555555555555ull
                                         : p.sW == 3 ? 0x9249249249249249ull
                                                     : 0x1111111111111111ull;      // (bits j with j % sW == 0)
        for (int w = c0, yy = y0, col = col0; w < c1; w += 4) {
            unsigned long long mw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) mw[j] = w + j < c1 ? cur[w + j] : 0ull;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (w + j >= c1) continue;
                if ((w + j) % CBG_GRID == (int)blockIdx.x) {      // (the grid is CBG_GRID workgroups)
                    copy[w + j] = mw[j];
                    other[w + j] = 0ull;
                }
                // the row phase is fixed per word, the column phases are sW fixed bit patterns shifted by the word's
                // first column
                const int ry = cbt_mod_s(yy + p.pH, p.sH), cs = cbt_mod_s(col * 64 + p.pW, p.sW);
                int c[CBT_MAX_S];
#pragma unroll
                for (int rx = 0; rx < CBT_MAX_S; ++rx) c[rx] = __popcll(mw[j] & (every << (rx < cs ? rx - cs + p.sW : rx - cs)));
#pragma unroll
                for (int ph = 0; ph < CBT_MAX_PH; ++ph) {
                    const int r = cbt_div_s(ph, p.sW), rx = ph - r * p.sW;
                    cnt[ph] += r == ry ? (rx == 0 ? c[0] : rx == 1 ? c[1] : rx == 2 ? c[2] : c[3]) : 0;
                }
                if (++col == p.L.wpr) col = 0, ++yy;
            }
        }
    } else {
        for (int i = c0; i < c1; i += 4) {
            int e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = i + j < c1 ? p.L.list[i + j] : -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int phE = cbt_phase_of(p, e[j]);
#pragma unroll
                for (int ph = 0; ph < CBT_MAX_PH; ++ph) cnt[ph] += phE == ph;
            }
        }
    }
    // the totals per phase (a phase without a tap counts nothing): wave sums by lane exchange, then the four waves
#pragma unroll
    for (int ph = 0; ph < CBT_MAX_PH; ++ph) {
        if (ph < P) {      // (uniform)
            if (!p.ckkP[ph]) cnt[ph] = 0;
            int sum = cnt[ph];
#pragma unroll
            for (int dlt = 32; dlt >= 1; dlt >>= 1) sum += __shfl_xor(sum, dlt, 64);
            if (lane == 0) sWaveTot[wave][ph] = sum;
        }
    }
    __syncthreads();
    if (t < CBT_MAX_PH) sTot[t] = t < P ? sWaveTot[0][t] + sWaveTot[1][t] + sWaveTot[2][t] + sWaveTot[3][t] : 0;
    if (cur)      // every workgroup has read the parity and the mask by now
        cb_flip_parity_last((int*)(p.L.frameMasks + 2 * words), par, G);
    else
        __syncthreads();

    // inclusive prefix over the 256 chunks of their numbers of listed pixels of phase ph -> sPre
    auto prefix = [&](int ph) {
        int inc = 0;
#pragma unroll
        for (int i = 0; i < CBT_MAX_PH; ++i) inc = i == ph ? cnt[i] : inc;
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int up = __shfl_up(inc, dlt, 64);
            if (lane >= dlt) inc += up;
        }
        __syncthreads();      // (the readers of the table before this one are done)
        if (lane == 63) sWave[wave] = inc;
        __syncthreads();
        for (int i = 0; i < wave; ++i) inc += sWave[i];
        sPre[t + 1] = inc;
        if (t == 0) sPre[0] = 0;
        __syncthreads();
    };
    int curPh = -1;

    // ---- work items: per phase (pixel tile, channel tile, k-slice); the k-split of a phase is capped by its stages
    const int tilesM = p.KP / CBG_BM;
    int base = 0;
    for (int ph = 0; ph < P; ++ph) base += (__builtin_amdgcn_readfirstlane(sTot[ph]) + CBG_BN - 1) / CBG_BN * tilesM;
    if (base == 0) return;
    int SKmax = 1;
    if (p.ws.slabs && base < G) SKmax = min(G / base, CBG_SKMAX);
    int items = 0;
    for (int ph = 0; ph < P; ++ph)
        items += (__builtin_amdgcn_readfirstlane(sTot[ph]) + CBG_BN - 1) / CBG_BN * tilesM *
                 max(1, min(SKmax, p.ckkP[ph] / CBG_BK));
    // (SKmax > 1: items <= base SKmax <= G, one item and one slab per workgroup)

    const int gn = t & 63, gk = wave * 8;      // the thread's place in the tile (cb_geom_stage.h)
    const int am = t >> 2, ak = (t & 3) * 8;
    const int wm = wave & 1, wn = wave >> 1;
    const T* src = (const T*)p.src;

    for (int item = blockIdx.x; item < items; item += G) {
        int ph = 0, rem = item, SK = 1, stages = 0, tileBase = 0, nPh = 0;
        for (; ph < P; ++ph) {
            nPh = __builtin_amdgcn_readfirstlane(sTot[ph]);
            const int tiles = (nPh + CBG_BN - 1) / CBG_BN * tilesM;
            stages = p.ckkP[ph] / CBG_BK;
            SK = max(1, min(SKmax, stages));
            if (rem < tiles * SK) break;
            rem -= tiles * SK;
            tileBase += tiles;
        }
        const int slice = rem % SK, tm = (rem / SK) % tilesM, tn = rem / (SK * tilesM);
        const int s0 = (int)((long)stages * slice / SK), s1 = (int)((long)stages * (slice + 1) / SK);
        const int CkkP = p.ckkP[ph];
        if (ph != curPh) prefix(ph), curPh = ph;
        __syncthreads();
        if (t < CBG_BN) {
            const int q = tn * CBG_BN + t;
            int pix = -1;
            if (q < nPh) {
                int lo = 0, hi = 255;      // last thread chunk whose prefix is <= q
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (sPre[mid] <= q) lo = mid; else hi = mid - 1;
                }
                int r = q - sPre[lo];
                int w = (int)min((long)total, (long)lo * chunk);
                const int wEnd = min(total, w + chunk);
                if (cur) {
                    const int ry = cbt_div_s(ph, p.sW), rx = ph - ry * p.sW;
                    int yy = w / p.L.wpr, col = w - yy * p.L.wpr;
                    unsigned long long mw = 0ull;
                    for (; w < wEnd; ++w) {
                        mw = cur[w] & cbt_phase_bits(p, ry, rx, yy, col);
                        const int c = __popcll(mw);
                        if (r < c) break;
                        r -= c;
                        if (++col == p.L.wpr) col = 0, ++yy;
                    }
                    if (w < wEnd) pix = yy * p.Wo + col * 64 + cb_select_bit(mw, r);
                } else {
                    for (; w < wEnd && pix < 0; w += 4) {      // (four loads in flight)
                        int e[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) e[j] = w + j < wEnd ? p.L.list[w + j] : -1;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (pix < 0 && cbt_phase_of(p, e[j]) == ph && r-- == 0) pix = e[j];
                    }
                }
                if (pix < 0 || pix >= HWo) pix = -1;      // (a foreign list is not trusted with addresses)
            }
            sList[t] = pix;
        }
        __syncthreads();

        const int pix = sList[gn];
        int oy = 0, ox = 0;
        if (pix >= 0) cbt_row_col(p, pix, oy, ox);
        const int iy0 = cbt_div_s(oy + p.pH, p.sH), ix0 = cbt_div_s(ox + p.pW, p.sW);      // the base input pixel
        const char* pbase = (const char*)(src + (long)iy0 * p.Wi + ix0);
        const T* wph = (const T*)(p.prepared + p.wOff[ph]);
        const int* tabPh = (const int*)(wph + (long)p.KP * CkkP);
        const T* wrow = wph + ((long)tm * CBG_BM + am) * CkkP + ak;
        CBG_TILE_STAGES(acc, wrow, tabPh, CkkP, pbase, pix, iy0, ix0, p.Hi, p.Wi, s0, s1)
        if (SK > 1)
            CBG_SPLITK_HANDOFF(acc, p.ws.slabs, p.ws.tickets + (tileBase + tn * tilesM + tm), item, slice, SK, sLast, continue)
        CBG_TILE_STORE(acc, sList, tm, p.bias, p.out, p.K, HWo, p.relu)
    }
}

bool cbt_arith_ok(int dtype) { return dtype == CB_F32 || dtype == CB_F16 || dtype == CB_F32S; }

}  // namespace

extern "C" {

int cbinfer_tconv_out_size(int Hi, int Wi, const cbTGeom* geom, int* Ho, int* Wo) {
    CB_REQUIRE(Ho && Wo);
    long ho, wo;
    const int st = cbt_out_size(Hi, Wi, geom, &ho, &wo);
    if (st != CB_OK) return st;
    CB_REQUIRE(ho <= 0x7fffffffl && wo <= 0x7fffffffl);
    *Ho = (int)ho, *Wo = (int)wo;
    return CB_OK;
}

long cbinfer_tconv_prepared_weights_bytes(int K, int C, const cbTGeom* geom, int dtype) {
    if (cbt_geom_status(geom) != CB_OK || K < 1 || C < 1 || !cbt_arith_ok(dtype)) return 0;
    return cbt_layout(K, C, geom, dtype).total;
}

long cbinfer_tconv_workspace_bytes(void) { return cbg_workspace_bytes(); }

int cbinfer_tconv_prep_weights(const void* weight, void* prepared, int K, int C, int Hi, int Wi, const cbTGeom* geom,
                               int dtype, cbStream_t stream) {
    CB_REQUIRE(weight && prepared && cbt_arith_ok(dtype));
    int Ho, Wo;
    const int st = cbt_shape(C, K, Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    const TConvLayout L = cbt_layout(K, C, geom, dtype);
    int most = 0;
    for (int ph = 0; ph < geom->sH * geom->sW; ++ph) most = most > L.ckkP[ph] ? most : L.ckkP[ph];
    if (most == 0) return CB_OK;
    const int KP = cbg_kpad(K);
    dim3 grid(cb_div_up((long)KP * most, 256), geom->sH * geom->sW), block(256);
    if (dtype == CB_F16)
        hipLaunchKernelGGL(cbt_prep_kernel<cb_half>, grid, block, 0, (hipStream_t)stream, (const cb_half*)weight,
                           (char*)prepared, K, C, KP, Hi, Wi, *geom, L);
    else
        hipLaunchKernelGGL(cbt_prep_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)weight,
                           (char*)prepared, K, C, KP, Hi, Wi, *geom, L);
    return cb_launch_status();
}

int cbinfer_change_detection_tconv(const void* input, void* state, uint64_t* frameMasks, int C, int Hi, int Wi,
                                   const cbTGeom* geom, float threshold, int updateInputState, int dtype,
                                   cbStream_t stream) {
    CB_REQUIRE(input && state && frameMasks);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(updateInputState >= 0 && updateInputState <= 2);
    int Ho, Wo;
    const int st = cbt_shape(C, 1, Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    if (Hi > 65535) return CB_ERR_UNSUPPORTED;      // (one grid row per input row)
    return cbg_launch_detect(cbt_detect_kernel<float>, cbt_detect_kernel<cb_half>, input, state, frameMasks, C, Hi, Wi,
                             Ho, Wo, *geom, threshold, updateInputState, dtype, (hipStream_t)stream);
}

int cbinfer_conv_changed_tconv(const void* input, const int32_t* changeList, int numChanges, const int32_t* countDev,
                               uint64_t* frameMasks, const void* prepared, const void* bias, void* output, int C, int Hi,
                               int Wi, int K, const cbTGeom* geom, int relu, void* workspace, int dtype,
                               cbStream_t stream) {
    CB_REQUIRE(input && prepared && output && cbt_arith_ok(dtype));
    int Ho, Wo;
    const int st = cbt_shape(C, K, Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    TConvParams p = {};
    const int ls = cbg_list_args(p.L, changeList, numChanges, countDev, frameMasks, !countDev, Ho, Wo);
    if (ls != CB_OK || cbg_nothing_listed(p.L)) return ls;
    const TConvLayout L = cbt_layout(K, C, geom, dtype);
    for (int ph = 0; ph < CBT_MAX_PH; ++ph) p.ckkP[ph] = L.ckkP[ph], p.wOff[ph] = L.wOff[ph];
    p.prepared = (const char*)prepared;
    p.KP = cbg_kpad(K);
    p.src = input, p.bias = bias, p.out = output;
    p.ws = cbg_workspace(workspace);
    p.K = K, p.Hi = Hi, p.Wi = Wi, p.Ho = Ho, p.Wo = Wo, p.relu = relu;
    p.sH = geom->sH, p.sW = geom->sW, p.pH = geom->pH, p.pW = geom->pW;
    p.rWo = 1.0 / Wo;
    cbg_dispatch_arith(dtype, [&](auto a) {
        hipLaunchKernelGGL((cbt_conv_kernel<typename decltype(a)::T, decltype(a)::ARITH>), dim3(CBG_GRID), dim3(256), 0,
                           (hipStream_t)stream, p);
    });
    return cb_launch_status();
}

int cbinfer_cbconvtranspose2d_forward(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                                      const void* prepared, const void* bias, int C, int Hi, int Wi, int K,
                                      const cbTGeom* geom, float threshold, int feedbackLoop, int copyInput, int relu,
                                      void* workspace, int dtype, cbStream_t stream) {
    CB_REQUIRE(input && prevInput && prevOutput && frameMasks && prepared && cbt_arith_ok(dtype));
    int Ho, Wo;
    int st = cbt_shape(C, K, Hi, Wi, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    const CbgFrameMode fm = cbg_frame_mode(input, prevInput, feedbackLoop, copyInput, dtype);
    st = cbinfer_change_detection_tconv(input, prevInput, frameMasks, C, Hi, Wi, geom, threshold, fm.update, fm.edt, stream);
    if (st != CB_OK) return st;
    return cbinfer_conv_changed_tconv(fm.src, nullptr, 0, nullptr, frameMasks, prepared, bias, prevOutput, C, Hi, Wi, K,
                                      geom, relu, workspace, dtype, stream);
}

}  // extern "C"
