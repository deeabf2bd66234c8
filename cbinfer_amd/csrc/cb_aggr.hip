// Change-based per-pixel kernel application on gfx950: the operator that takes a volume of per-pixel
// weights back to a feature map -- the attn . V half of neighbourhood attention, the kernel application of
// kernel-prediction networks, CARAFE's reassembly, involution, dynamic filters --
//   out[c, y, x] = sum_{i < Dy, j < Dx} w[g(c) T + i Dx + j, y, x] * v[c, y + y0 + i step, x + x0 + j step],
// T = Dy Dx, g(c) = c / (C / G), a tap outside the map contributing nothing.  The reference has no such operator; the
// contract and the arithmetic are in include/cbinfer_hip.h, which is the specification.  out[:, y, x] can differ from
// last frame's only if w changed at (y, x) or v changed at one of the window's taps: the footprint of cb_corr.hip with
// a := w, b := v, whose word, list launches and clearing launch cb_window.h holds for both.  A frame is
//   per operand in LIST form, one launch in front; for v in LIST form, one launch behind (cb_window.h);
//   one launch, the whole-word walk of cb_maskwalk.h over the output mask.  The unit: the word's row y and 64 columns
//              are four 16-pixel GROUPS, one per wave; a group without a listed pixel multiplies nothing, a group with
//              one is computed WHOLE and only its listed pixels are stored, so a pixel's bits depend on its own
//              operands and on x mod 16 alone.  The roles on the matrix unit are M = 16 channels, N = the group's 16
//              pixels, K = the 16 NT columns of v's row y + dy that the group's windows span:
//                B, the band of displacement row i: Band[col, n] = w[g T + i Dx + j, y, xg + n] where col - n = j step,
//                   0 <= j < Dx, else +0.  It is built IN REGISTERS, without LDS: a lane's element of k-step s is one
//                   predicated global load (f16: the 8 consecutive k of a lane are 8 planes, 8 such loads) -- the
//                   loads of a wave walk the diagonals of Dx planes' 64-byte (32-byte) runs, every element of which
//                   is wanted exactly once --, 4 NT registers per row, reused over the channel tiles of the pass.
//                A, the strip of v: per (displacement row, channel block of 64 inside one group) the 256 threads stage
//                   channels x (3 + NT) tiles from column xw + x0 into LDS by row-segment loads, zero for a column
//                   outside the map and a channel outside the block, and only the tiles that a group with a listed
//                   pixel reads.  f32: [channel tile][column][16 channels], a column padded to 17 words: the staging
//                   write (lanes along the columns) and the fragment read (64 lanes on 4 columns x 16 channels) are
//                   conflict-free.  f16: [column / 8][64 channels][8 columns], a column group padded by one entry.
//                   The four waves read the overlapping tile ranges wave .. wave + NT - 1 of the one strip.
//              Loop order: weight group -> channel block -> displacement row -> k, the 4 x 4 accumulator registers of
//              the block live across all rows; a row wholly outside the map issues nothing.  The C/D layout has the
//              pixel on lane & 15 and the channel on 4 (lane >> 4) + r: the result is rounded once and stored straight
//              from the registers, one run of 16 pixels per channel plane, predicated on the group's mask bits.
// Every column of the strip is multiplied, the off-band ones by +0: the operands must be FINITE (the header says so).
// No host sync, memset, allocation, data atomics or inline assembly; all stores are plain vector stores.
#include <type_traits>

#include "cb_window.h"

namespace {

#define CBA_MAXPLANES 4096
#define CBA_CB 64      // channels of a block: four accumulator tiles

struct cba_geo {
    int C, H, W, G, Cg, T, NT, NTE;      // NTE: NT with K padded to the dtype's k-step (f16: even)
    unsigned inv;                          // ceil(2^16 / step): d / step == (d inv) >> 16 for 0 <= d < 2^13
    cbw_window win;
};

// the LDS strip of a dtype for NTMAX tiles per group: COLS columns, WORDS elements
template <typename T, int NTMAX>
struct cba_strip;
template <int NTMAX>
struct cba_strip<float, NTMAX> {
    static constexpr int NTE = NTMAX, COLS = 16 * (3 + NTE), WORDS = 4 * COLS * 17;
};
template <int NTMAX>
struct cba_strip<cb_half, NTMAX> {
    static constexpr int NTE = NTMAX + (NTMAX & 1), COLS = 16 * (3 + NTE), WORDS = (COLS / 8) * (CBA_CB + 1) * 8;
};

// Stage nct channel tiles x `tiles` 16-column tiles of one map row into dst: channel ch < nch (zero from there to
// 16 nct) of the block whose plane 0 row starts at `row`, column xs + col (zero outside [0, W)).  Only tiles whose bit
// is set in `need` are written (and only those are read afterwards).  f32: consecutive threads take consecutive
// columns of one channel; dst[((ch / 16) COLS + col) 17 + ch % 16].
template <int COLS>
__device__ __forceinline__ void cba_stage(float* __restrict__ dst, const float* __restrict__ row, long HW, int nch,
                                          int nct, int xs, int W, int tiles, unsigned need) {
    const int cols = tiles * 16, total = nct * 16 * cols;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ch = e / cols, col = e - ch * cols;
        if (!((need >> (col >> 4)) & 1u)) continue;
        const int x = xs + col;
        // (an address is formed only inside the map and the block)
        const float val = (x >= 0 && x < W && ch < nch) ? row[(long)ch * HW + x] : 0.f;
        dst[((ch >> 4) * COLS + col) * 17 + (ch & 15)] = val;
    }
}
// f16: consecutive threads take consecutive groups of 8 columns of one channel; dst[((col / 8) 65 + ch) 8 + col % 8].
template <int COLS>
__device__ __forceinline__ void cba_stage(cb_half* __restrict__ dst, const cb_half* __restrict__ row, long HW, int nch,
                                          int nct, int xs, int W, int tiles, unsigned need) {
    const int ncg = tiles * 2, total = nct * 16 * ncg;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ch = e / ncg, cg = e - ch * ncg;
        if (!((need >> (cg >> 1)) & 1u)) continue;
        halfx8 p;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int x = xs + cg * 8 + i;
            p[i] = (x >= 0 && x < W && ch < nch) ? row[(long)ch * HW + x] : cb_half(0);
        }
        *(halfx8*)&dst[(cg * (CBA_CB + 1) + ch) * 8] = p;
    }
}

// One element of the band: column `col` of the group's K axis for pixel n -- w's plane j at the pixel where
// col - n = j step with 0 <= j < Dx and the pixel is one of the row (pix), else +0.  wrow: the group's first pixel in
// plane 0 of displacement row i.
template <typename T>
__device__ __forceinline__ T cba_band(const T* __restrict__ wrow, long HW, int col, int n, bool pix, const cba_geo& g) {
    const int d = col - n;
    const int j = d >= 0 ? (int)(((unsigned)d * g.inv) >> 16) : 0;
    const bool on = pix && d >= 0 && j * g.win.step == d && j < g.win.Dx;
    return on ? wrow[(long)j * HW + n] : T(0);
}

// w [G T, H, W], v and out [C, H, W].  maskW / maskV / all as cbc_corr_kernel's maskA / maskB / all.  NTMAX >= g.NT
// sizes the band registers and the LDS.
template <typename T, int NTMAX>
__global__ __launch_bounds__(256) void cba_aggr_kernel(const T* __restrict__ w, const T* __restrict__ v,
                                                      T* __restrict__ out,
                                                      const unsigned long long* __restrict__ maskW,
                                                      const unsigned long long* __restrict__ maskV, int all,
                                                      unsigned long long* bits,
                                                      unsigned long long* __restrict__ maskCopy, long words, cba_geo g,
                                                      int wpr) {
    using strip = cba_strip<T, NTMAX>;
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int KSTEPS = F16 ? strip::NTE / 2 : 4 * strip::NTE;      // k-steps of a displacement row
    using frag = typename std::conditional<F16, halfx8, float>::type;   // a lane's operand of one k-step
    __shared__ __attribute__((aligned(16))) T sV[strip::WORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, q = lane >> 4;
    const long HW = (long)g.H * g.W;
    const int ksteps = F16 ? g.NTE / 2 : 4 * g.NTE;
    cb_walk_word_units(
        bits, maskCopy, words, g.W, wpr, all,
        [&](long wd, int y, int tile) -> unsigned long long {
            if (all) return 0ull;
            return cbw_footprint_word(maskW, maskV, wd, y, tile, g.H, wpr, g.win, lane);
        },
        [&](unsigned long long word, int y, int tile) {
            const int xw = tile * 64, xg = xw + 16 * wave;
            // this wave's group, and the tiles of the strip that the groups with a listed pixel read
            const unsigned grp = __builtin_amdgcn_readfirstlane((unsigned)(word >> (16 * wave)) & 0xffffu);
            unsigned need = 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if ((word >> (16 * u)) & 0xffffull) need |= ((1u << g.NTE) - 1u) << u;
            const bool pix = xg + n < g.W;                 // (a group may be cut by the row end)
            const bool listed = (grp >> n) & 1u;           // (a set bit is a pixel of the row: cb_valid_mask)
            for (int gi = 0; gi < g.G; ++gi)
                for (int cb = 0; cb < g.Cg; cb += CBA_CB) {
                    const int c0 = gi * g.Cg + cb, nch = min(CBA_CB, g.Cg - cb), nct = (nch + 15) >> 4;
                    floatx4 acc[4];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
                    for (int di = 0; di < g.win.Dy; ++di) {
                        const int yy = y + g.win.y0 + di * g.win.step;
                        if (yy < 0 || yy >= g.H) continue;      // (uniform: a row wholly outside issues nothing)
                        __syncthreads();      // the fragments of the row before have been read
                        cba_stage<strip::COLS>(sV, v + (long)c0 * HW + (long)yy * g.W, HW, nch, nct, xw + g.win.x0, g.W,
                                               3 + g.NTE, need);
                        // the band of this row, in registers (wave-uniform test; the barriers are outside it)
                        frag band[KSTEPS];
                        if (grp != 0u) {
                            const T* wrow = w + ((long)gi * g.T + (long)di * g.win.Dx) * HW + (long)y * g.W + xg;
#pragma unroll
                            for (int s = 0; s < KSTEPS; ++s) {
                                if (s >= ksteps) continue;
                                if constexpr (F16) {
#pragma unroll
                                    for (int e = 0; e < 8; ++e)
                                        band[s][e] = cba_band<T>(wrow, HW, 32 * s + 8 * q + e, n, pix, g);
                                } else {
                                    band[s] = cba_band<T>(wrow, HW, 4 * s + q, n, pix, g);
                                }
                            }
                        }
                        __syncthreads();
                        if (grp == 0u) continue;
#pragma unroll
                        for (int s = 0; s < KSTEPS; ++s) {
                            if (s >= ksteps) continue;
#pragma unroll
                            for (int ct = 0; ct < 4; ++ct) {
                                if (ct >= nct) continue;
                                if constexpr (F16) {
                                    const halfx8 av =
                                        *(const halfx8*)&sV[((2 * wave + 4 * s + q) * (CBA_CB + 1) + 16 * ct + n) * 8];
                                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, band[s], acc[ct], 0, 0, 0);
                                } else {
                                    const float av = sV[(ct * strip::COLS + 16 * wave + 4 * s + q) * 17 + n];
                                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, band[s], acc[ct], 0, 0, 0);
                                }
                            }
                        }
                    }
                    // C/D layout of the 16x16 MFMAs: pixel lane & 15, channel 4 (lane >> 4) + register
                    if (grp != 0u && listed) {
                        T* o = out + (long)c0 * HW + (long)y * g.W + xg + n;
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int ch = 16 * ct + 4 * q + r;
                                if (ch < nch) o[(long)ch * HW] = (T)acc[ct][r];      // the one rounding to the dtype
                            }
                    }
                }
        });
}

template <typename T>
void cba_launch(const void* w, const void* v, void* out, const uint64_t* maskW, const uint64_t* maskV, int all,
                uint64_t* bits, uint64_t* maskCopy, cba_geo g, hipStream_t s) {
    const int wpr = (g.W + 63) / 64;
    const long words = (long)g.H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
    g.NTE = sizeof(T) == 2 ? g.NT + (g.NT & 1) : g.NT;
#define CBA_GO(NTMAX)                                                                                                  \
    hipLaunchKernelGGL((cba_aggr_kernel<T, NTMAX>), grid, block, 0, s, (const T*)w, (const T*)v, (T*)out,               \
                       (const unsigned long long*)maskW, (const unsigned long long*)maskV, all,                        \
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, g, wpr)
    if (g.NT <= 2)
        CBA_GO(2);
    else if (g.NT <= 4)
        CBA_GO(4);
    else
        CBA_GO(9);
#undef CBA_GO
}

}  // namespace

int cbinfer_aggregate_supported(const cbAggr* a, int C, int H, int W) {
    if (!a || !cbw_window_ok(a->y0, a->y1, a->x0, a->x1, a->step)) return 0;
    const long T = (long)((a->y1 - a->y0) / a->step + 1) * ((a->x1 - a->x0) / a->step + 1);
    if (!(a->groups >= 1 && C >= 1 && H >= 1 && W >= 1 && C % a->groups == 0 && a->groups * T <= CBA_MAXPLANES)) return 0;
    // (a list addresses a pixel with an int32; the larger of the two plane counts is within the other operators' limit)
    const long planes = a->groups * T > C ? a->groups * T : C;
    return (long)H * W < (1l << 31) && planes * 64 < (1l << 31);
}

int cbinfer_cbaggregate_forward(const void* w, const void* v, void* outputState, const uint64_t* maskW,
                                const int32_t* listW, int capW, const int32_t* countW, const uint64_t* maskV,
                                const int32_t* listV, int capV, const int32_t* countV, uint64_t* vBits, uint64_t* bits,
                                uint64_t* maskCopy, int C, int H, int W, const cbAggr* aggr, int dtype,
                                cbStream_t stream) {
    // (every argument is checked before the first launch)
    const cbw_forms f = {maskW, listW, capW, countW, maskV, listV, capV, countV, vBits, bits, maskCopy};
    CB_REQUIRE(w && v && outputState && outputState != w && outputState != v);
    CB_REQUIRE(cbw_forms_ok(f));
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_aggregate_supported(aggr, C, H, W));
    cba_geo g;
    g.C = C, g.H = H, g.W = W, g.G = aggr->groups, g.Cg = C / aggr->groups;
    g.win.y0 = aggr->y0, g.win.x0 = aggr->x0, g.win.step = aggr->step;
    g.win.Dy = (aggr->y1 - aggr->y0) / aggr->step + 1;
    g.win.Dx = (aggr->x1 - aggr->x0) / aggr->step + 1;
    g.T = g.win.Dy * g.win.Dx;
    g.NT = g.NTE = (16 + aggr->x1 - aggr->x0 + 15) / 16;      // (at most 9)
    g.inv = (65536u + aggr->step - 1) / aggr->step;
    const hipStream_t s = (hipStream_t)stream;
    cbw_frame fr;
    int st = cbw_lists_to_bits(f, H, W, stream, &fr);
    if (st != CB_OK) return st;
    cb_dispatch_dtype(dtype, [&](auto t) {
        cba_launch<decltype(t)>(w, v, outputState, fr.mA, fr.mB, fr.all, bits, maskCopy, g, s);
    });
    st = cb_launch_status();
    return (st != CB_OK || !fr.bList) ? st : cbw_clear_list(f, H, W, s);
}
