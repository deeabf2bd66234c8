// Change-based resize to any size (nearest, nearest-exact, bilinear, bicubic; up and down, 1/8 .. 8 per axis) on gfx950
// (DESIGN 5.23): F.interpolate(x, size=...) of segmentation heads, FPN top-down steps, HRNet fuse layers and bicubic
// depth / super-resolution heads.  The reference has no such operator; the contract, the source rules and the order of
// the f32 arithmetic are in include/cbinfer_hip.h, which is the specification.  An output pixel reads 1, 2x2 or 4x4
// input pixels at coordinates that are a rational function of its own, and every producer of this library leaves the
// pixels outside its change list bit for bit as they were: recomputing at the FOOTPRINT of the input's changes gives
// the dense result exactly, without a threshold.  A frame is cb_decoder.hip's with a general source function:
//   an input in LIST form, one launch in front: one thread per (entry, candidate output row) ORs the output pixels that
//              read the entry into the zeroed working mask of the OUTPUT map, at most two 64-bit atomicOr per row;
//   one launch, mask-driven: the word walk of cb_maskwalk.h (cb_walk_words) over the output mask.  Lane j of every wave
//              owns output column 64 w + j of the word and tests the input change bits of the taps of its own column
//              against the word's tap rows -- each lane reads the input words of its own taps, a word that is
//              downscaled spans up to eight of them --, one ballot makes the word.
// No host sync, memset, allocation, data atomics or inline assembly.
#include "cb_maskwalk.h"

// hipcc contracts a * b + c to an FMA by default, and its __fmul_rn / __fadd_rn are plain operators of a header that is
// compiled with that default: they fuse as well.  So the arithmetic below is written with operators under this file's
// pragma: everything is evaluated as written, one rounding per operation (as cb_chanreduce.hip).
#pragma clang fp contract(off)

namespace {

#define CBR_MAXSTEP 8        // 1/8 <= a / b <= 8 per axis
#define CBR_MAXTERM 4096     // a, b
#define CBR_MAXEXT (1 << 15)

// KIND 0: nearest; 1: nearest-exact; 2: linear; 3: cubic.  One axis: n input and N output pixels, the step a / b.
struct cbr_axis {
    int n, N, a, b;
};

template <int KIND>
struct cbr_kind {
    static constexpr int taps = KIND < 2 ? 1 : (KIND == 2 ? 2 : 4);
};

// The taps (input coordinates, clamped to the map) of output coordinate o, and numerator rho and denominator den of
// the weight fraction t -- all in integers, the header's rules.  Within the limits the entry point checks (extents below
// 2^15, a and b at most 4096) every intermediate fits an int32 -- (2 o + 1) a < 2^16 2^12, o (n - 1) < 2^30, num >= -b --
// so the 64-bit intermediates of the header are not needed, and a 32-bit division costs a fraction of a 64-bit one.
// Linear clamps both taps to n - 1, which never acts within the limits (N a <= n b keeps the last source coordinate
// below n - 1/2).
template <int KIND>
__device__ __forceinline__ void cbr_source(int o, const cbr_axis& ax, int align, int (&tap)[4], int& rho, int& den) {
    rho = 0, den = 1;
    if (KIND == 0) {
        tap[0] = min((int)((unsigned)(o * ax.a) / (unsigned)ax.b), ax.n - 1);
        return;
    }
    if (KIND == 1) {
        tap[0] = min((int)((unsigned)((2 * o + 1) * ax.a) / (unsigned)(2 * ax.b)), ax.n - 1);
        return;
    }
    int num;
    if (!align) {
        num = (2 * o + 1) * ax.a - ax.b;
        den = 2 * ax.b;
    } else {
        num = ax.N > 1 ? o * (ax.n - 1) : 0;
        den = ax.N > 1 ? ax.N - 1 : 1;
    }
    if (KIND == 2) {
        num = max(num, 0);
        const int i0 = (int)((unsigned)num / (unsigned)den);
        rho = num - i0 * den;
        tap[0] = min(i0, ax.n - 1);
        tap[1] = min(i0 + 1, ax.n - 1);
    } else {
        // floor: a negative num is >= -b > -den, so its quotient is -1
        const int i0 = num >= 0 ? (int)((unsigned)num / (unsigned)den) : -1;
        rho = num - i0 * den;
#pragma unroll
        for (int k = 0; k < 4; ++k) tap[k] = min(max(i0 - 1 + k, 0), ax.n - 1);
    }
}

template <int KIND>
__device__ __forceinline__ bool cbr_reads(const int (&tap)[4], int i) {
    bool hit = false;
#pragma unroll
    for (int k = 0; k < cbr_kind<KIND>::taps; ++k) hit |= tap[k] == i;
    return hit;
}

// floor(v q) for the rational q = qb / qa, v of either sign (|v| < 2^15, qb < 2^15: an int32 holds the product)
__device__ __forceinline__ int cbr_floor_mul(int v, int qb, int qa) {
    const int p = v * qb;
    return p >= 0 ? p / qa : -((-p + qa - 1) / qa);
}

// List form: one thread per (list entry, r-th candidate output row), r < RH.  The candidates of input coordinate y on
// an axis are the RH = ceil(6 q) + 3 output coordinates from floor((y - 3) q) - 1 on, with q = qb / qa output pixels per
// input pixel: b / a without align_corners, N / n with it (the launcher's choice; q <= 8 either way, so a row has at
// most 51 candidate columns: two words).  They hold every output coordinate o that reads y:
//   the source coordinate is s(o) = (o + d) / q - e with (d, e) = (0, 0) nearest, (1/2, 0) nearest-exact, (1/2, 1/2)
//   linear / cubic, or s(o) = o (n - 1) / (N - 1) with align_corners.  The unclamped taps lie in [floor(s) - 1,
//   floor(s) + 2], so o reads y only if y - 2 <= s(o) < y + 2: a tap clamped to 0 has s < 1, one clamped to n - 1 has
//   s >= n - 2, and N a <= n b (cbinfer_resize_supported) keeps s(N - 1) < n - 1/2, so clamping admits nothing further.
//   Without align_corners that is (y - 2) q - 1/2 <= o < (y + 5/2) q.  The first candidate is <= (y - 3) q - 1, below
//   the lower end; the last is > (y - 3) q - 2 + 6 q + 2 = (y + 3) q, beyond the upper one.
//   With align_corners and n, N >= 2, (y - 2) / z <= o < (y + 2) / z with z = (n - 1) / (N - 1) and q = N / n.
//   Upscaling, 1 / z >= q: the lower end is >= (y - 2) q; the upper end is (y + 2) q + (y + 2)(N - n) / (n (n - 1)),
//   which is <= (y + 3) q when y + 3 <= n - 1, and otherwise N - 1 <= (y + 3) N / n bounds o.  Downscaling,
//   1 / z = q - (n - N) / (n (n - 1)) <= q: the upper end is <= (y + 2) q and the lower end >= (y - 2) q - 1.
//   n == 1 or N == 1: at most 8 output coordinates, all within [-3 q - 1, 3 q + 1].
// Every candidate is TESTED with cbr_source; the range only has to hold them all.  An input pixel that no output
// reads lists nothing.
template <int KIND>
__global__ __launch_bounds__(256) void cbr_footprint_list_kernel(const int32_t* __restrict__ list, int nHost,
                                                                const int32_t* __restrict__ countDev, cbr_axis axH,
                                                                cbr_axis axW, int align, int qaH, int qbH, int qaW,
                                                                int qbW, int RH, int RW, int wprO,
                                                                unsigned long long* __restrict__ bits) {
    const int N = countDev ? min(*countDev, nHost) : nHost;
    const long total = (long)N * RH;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int e = (int)(i / RH), r = (int)(i - (long)e * RH);
        const int pos = list[e];
        if ((unsigned)pos >= (unsigned)(axH.n * axW.n)) continue;      // (an out-of-map entry is dropped)
        const int y = pos / axW.n, x = pos - y * axW.n;
        const int oy = cbr_floor_mul(y - 3, qbH, qaH) - 1 + r;
        if (oy < 0 || oy >= axH.N) continue;
        int tap[4], rho, den;
        cbr_source<KIND>(oy, axH, align, tap, rho, den);
        if (!cbr_reads<KIND>(tap, y)) continue;
        const int first = cbr_floor_mul(x - 3, qbW, qaW) - 1;
        const int oxLo = max(first, 0), oxHi = min(first + RW - 1, axW.N - 1);
        const int w0 = oxLo >> 6;
        unsigned long long m0 = 0ull, m1 = 0ull;
        for (int ox = oxLo; ox <= oxHi; ++ox) {
            cbr_source<KIND>(ox, axW, align, tap, rho, den);
            if (cbr_reads<KIND>(tap, x)) {
                if ((ox >> 6) == w0)
                    m0 |= 1ull << (ox & 63);
                else
                    m1 |= 1ull << (ox & 63);
            }
        }
        if (m0) atomicOr(bits + (long)oy * wprO + w0, m0);
        if (m1) atomicOr(bits + (long)oy * wprO + w0 + 1, m1);
    }
}

// The cubic convolution weights, A = -0.75, of the header: cbr_w_near(t) for the taps at distance t <= 1 and
// cbr_w_far(s) for those at distance 1 <= s <= 2 (5 A = -3.75, 8 A = -6, 4 A = -3, A + 2 = 1.25, A + 3 = 2.25).
__device__ __forceinline__ float cbr_w_far(float s) {
    float m = -0.75f * s;
    m = m - -3.75f;
    m = m * s;
    m = m + -6.f;
    m = m * s;
    return m - -3.f;
}
__device__ __forceinline__ float cbr_w_near(float t) {
    float m = 1.25f * t;
    m = m - 2.25f;
    m = m * t;
    m = m * t;
    return m + 1.f;
}
// the weights of the KIND's taps from t = rho / den (one correctly rounded division)
template <int KIND>
__device__ __forceinline__ void cbr_weights(int rho, int den, float (&w)[4]) {
    const float t = __fdiv_rn((float)rho, (float)den);
    if (KIND == 2) {
        w[0] = 1.f - t;
        w[1] = t;
    } else {
        w[0] = cbr_w_far(t + 1.f);
        w[1] = cbr_w_near(t);
        w[2] = cbr_w_near(1.f - t);
        w[3] = cbr_w_far(2.f - t);
    }
}
// ((w0 p0 + w1 p1) + w2 p2) + w3 p3 over the KIND's taps, every product and sum rounded on its own
template <int KIND>
__device__ __forceinline__ float cbr_combine(const float (&w)[4], const float (&p)[4]) {
    float acc = w[0] * p[0];
#pragma unroll
    for (int k = 1; k < cbr_kind<KIND>::taps; ++k) {
        const float term = w[k] * p[k];
        acc = acc + term;
    }
    return acc;
}

// in [C, Hi, Wi], out [C, Ho, Wo].  inMask: the input's change mask of this frame (row-padded over the INPUT map), or
// NULL; all: the input lists every pixel.  An input in list form has its footprint in `bits` already.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void cbr_resize_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                        const unsigned long long* __restrict__ inMask, int all,
                                                        unsigned long long* bits,
                                                        unsigned long long* __restrict__ maskCopy, long words, int C,
                                                        cbr_axis axH, cbr_axis axW, int align, int wprI, int wprO) {
    constexpr int TAPS = cbr_kind<KIND>::taps;
    const long HWi = (long)axH.n * axW.n, HWo = (long)axH.N * axW.N;
    const int Wi = axW.n, Wo = axW.N;
    const int lane = threadIdx.x & 63;
    int ty[4];           // the tap rows of the word's output row: made by makeWord, read by the items
    float wy[4];         // and their weights
    cb_walk_words(
        bits, maskCopy, words, C, Wo, wprO, all,
        [&](long, int oy, int tile) {
            int rho, den;
            cbr_source<KIND>(oy, axH, align, ty, rho, den);
            if (KIND >= 2) cbr_weights<KIND>(rho, den, wy);
            if (!inMask) return 0ull;
            // every wave makes the same word: lane j tests the change bits of the taps of column 64 tile + j
            const int ox = tile * 64 + lane;
            bool bit = false;
            if (ox < Wo) {
                int tx[4];
                cbr_source<KIND>(ox, axW, align, tx, rho, den);
                unsigned long long m = 0ull;
#pragma unroll
                for (int j = 0; j < TAPS; ++j) {
                    unsigned long long col = 0ull;
#pragma unroll
                    for (int k = 0; k < TAPS; ++k) col |= inMask[(long)ty[k] * wprI + (tx[j] >> 6)];
                    m |= col >> (tx[j] & 63);
                }
                bit = (m & 1ull) != 0;
            }
            return (unsigned long long)__ballot(bit);
        },
        [&](int c, int oy, int ox) {
            int tx[4], rho, den;
            cbr_source<KIND>(ox, axW, align, tx, rho, den);
            const T* src = in + (long)c * HWi;
            T res;
            if (KIND < 2) {
                res = src[(long)ty[0] * Wi + tx[0]];      // (a copy: bit for bit)
            } else {
                // rows first over x, then over y; the value in f32, rounded to T once
                float wx[4], rows[4], p[4];
                cbr_weights<KIND>(rho, den, wx);
#pragma unroll
                for (int k = 0; k < TAPS; ++k) {
#pragma unroll
                    for (int j = 0; j < TAPS; ++j) p[j] = cb_load_f32(src + (long)ty[k] * Wi + tx[j]);
                    rows[k] = cbr_combine<KIND>(wx, p);
                }
                res = (T)cbr_combine<KIND>(wy, rows);
            }
            out[(long)c * HWo + (long)oy * Wo + ox] = res;
        });
}

inline int cbr_kind_of(const cbResize& r) {
    return r.mode == CB_RESIZE_NEAREST ? 0 : r.mode == CB_RESIZE_NEAREST_EXACT ? 1 : r.mode == CB_RESIZE_BILINEAR ? 2 : 3;
}

template <typename F>
inline void cbr_dispatch_kind(int kind, F f) {
    switch (kind) {
        case 0: f(std::integral_constant<int, 0>()); break;
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        default: f(std::integral_constant<int, 3>()); break;
    }
}

template <typename T>
void cbr_launch(const void* in, void* out, const uint64_t* inMask, int all, uint64_t* bits, uint64_t* maskCopy, int C,
                const cbr_axis& axH, const cbr_axis& axW, const cbResize& r, hipStream_t s) {
    const int wprO = (axW.N + 63) / 64, wprI = (axW.n + 63) / 64;
    const long words = (long)axH.N * wprO;
    const dim3 grid(cb_walk_grid(words)), block(256);
    cbr_dispatch_kind(cbr_kind_of(r), [&](auto k) {
        hipLaunchKernelGGL((cbr_resize_kernel<T, decltype(k)::value>), grid, block, 0, s, (const T*)in, (T*)out,
                           (const unsigned long long*)inMask, all, (unsigned long long*)bits,
                           (unsigned long long*)maskCopy, words, C, axH, axW, r.alignCorners, wprI, wprO);
    });
}

void cbr_launch_list(const int32_t* list, int cap, const int32_t* count, uint64_t* bits, const cbr_axis& axH,
                     const cbr_axis& axW, const cbResize& r, hipStream_t s) {
    // q = qb / qa output pixels per input pixel, the candidate ranges' measure (the kernel's comment)
    const int qaH = r.alignCorners ? axH.n : axH.a, qbH = r.alignCorners ? axH.N : axH.b;
    const int qaW = r.alignCorners ? axW.n : axW.a, qbW = r.alignCorners ? axW.N : axW.b;
    const int RH = (int)((6l * qbH + qaH - 1) / qaH) + 3, RW = (int)((6l * qbW + qaW - 1) / qaW) + 3;
    const int wprO = (axW.N + 63) / 64;
    long blocks = ((long)cap * RH + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    const dim3 grid((unsigned)blocks), block(256);
    cbr_dispatch_kind(cbr_kind_of(r), [&](auto k) {
        hipLaunchKernelGGL((cbr_footprint_list_kernel<decltype(k)::value>), grid, block, 0, s, list, cap, count, axH, axW,
                           r.alignCorners, qaH, qbH, qaW, qbW, RH, RW, wprO, (unsigned long long*)bits);
    });
}

// one axis within the limits of the header
inline bool cbr_axis_ok(int n, int N, int a, int b, bool stepUsed) {
    if (n < 1 || N < 1 || n >= CBR_MAXEXT || N >= CBR_MAXEXT) return false;
    if (a < 1 || b < 1 || a > CBR_MAXTERM || b > CBR_MAXTERM) return false;
    if (a > CBR_MAXSTEP * b || b > CBR_MAXSTEP * a) return false;
    if ((long)N * CBR_MAXSTEP < n || N > (long)n * CBR_MAXSTEP) return false;
    // the output map does not reach beyond the input: the last source coordinate stays inside it
    return !stepUsed || (long)N * a <= (long)n * b;
}

}  // namespace

int cbinfer_resize_supported(const cbResize* r, int Hi, int Wi) {
    if (!r) return 0;
    if (r->mode != CB_RESIZE_NEAREST && r->mode != CB_RESIZE_NEAREST_EXACT && r->mode != CB_RESIZE_BILINEAR &&
        r->mode != CB_RESIZE_BICUBIC)
        return 0;
    const bool nearest = r->mode == CB_RESIZE_NEAREST || r->mode == CB_RESIZE_NEAREST_EXACT;
    if (r->alignCorners != 0 && (r->alignCorners != 1 || nearest)) return 0;
    const bool stepUsed = r->alignCorners == 0;
    return cbr_axis_ok(Hi, r->Ho, r->aH, r->bH, stepUsed) && cbr_axis_ok(Wi, r->Wo, r->aW, r->bW, stepUsed) &&
           (long)r->Ho * r->Wo < (1l << 31);
}

int cbinfer_cbresize_forward(const void* input, void* outputState, const uint64_t* inputMask, const int32_t* list,
                             int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy, int C, int Hi, int Wi,
                             const cbResize* rs, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && outputState && bits && maskCopy && bits != maskCopy && C >= 1 && Hi >= 1 && Wi >= 1);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_resize_supported(rs, Hi, Wi));
    CB_REQUIRE(capN >= 0 && !(inputMask && list) && (list || !countDev));
    CB_REQUIRE(inputMask != bits && inputMask != maskCopy);
    // (a list addresses a pixel with an int32; the kernel numbers a word's items with an int)
    CB_REQUIRE((long)C * 64 < (1l << 31));
    const cbr_axis axH = {Hi, rs->Ho, rs->aH, rs->bH}, axW = {Wi, rs->Wo, rs->aW, rs->bW};
    const int all = !inputMask && !list;
    if (list && capN > 0) {
        cbr_launch_list(list, capN, countDev, bits, axH, axW, *rs, (hipStream_t)stream);
        const int st = cb_launch_status();
        if (st != CB_OK) return st;
    }
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbr_launch<decltype(t)>(input, outputState, inputMask, all, bits, maskCopy, C, axH, axW, *rs,
                                (hipStream_t)stream);
    });
    return cb_launch_status();
}
