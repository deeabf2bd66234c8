// Change-based grid sampling (F.grid_sample: nearest, bilinear, bicubic; zeros, border, reflection; a normalised grid or
// a flow field in pixels) on gfx950: fixed warps -- a homography, a rectification, an affine grid -- and
// flow warping of video networks.  The reference has no such operator; the contract and the order of the f32 arithmetic
// are in include/cbinfer_hip.h, which is the specification.  An output pixel reads 1, 2x2 or 4x4 input pixels at a
// position given by ITS OWN coordinate pair, and every producer of this library leaves the pixels outside its change
// list bit for bit as they were: the pixel can differ from last frame's only where its coordinates or one of its taps
// changed, and recomputing there is the dense result exactly, without a threshold.  cb_resize.hip inverts a rational
// source function analytically; here the function is DATA and cannot be inverted, so the frame is driven from the
// output side.  This is a gather, not a contraction: no matrix instruction fits.  A frame is
//   for an operand in LIST form, one launch in front (cb_list_to_bits of cb_maskwalk.h): the input's list into the
//              working mask of the INPUT map, the coordinates' list into the working mask of the OUTPUT map;
//   one launch, the whole-word walk of cb_maskwalk.h (cb_walk_word_units) over the output mask.  Per word, lane j of
//              every wave owns output pixel 64 tile + j: it loads its coordinate pair and derives taps and weights ONCE;
//              the tap ROWS are split over the four waves, each tests the input change bits of its row with 64-bit
//              gathers (a word is loaded again only where the next tap lies in another one), the four ballots are ORed
//              through LDS.  The listed lanes leave their pixel's record -- clamped tap offsets and weights, -1 for a
//              tap that does not count -- in LDS (at most 4 KB), and behind a barrier the 256 threads take the
//              (listed pixel, channel) items, listed pixel fastest: the coordinate arithmetic and the mask tests are
//              paid once per pixel, not once per channel, and for a smooth warp neighbouring lanes gather neighbouring
//              addresses;
//   for an input in LIST form, one launch behind: zero to the words of the input working mask that the list named
//              (the frame launch reads that mask from every workgroup, so it cannot clear it itself).
// No host sync, memset, allocation, data atomics or inline assembly; all stores are plain vector stores.
#include "cb_maskwalk.h"

// hipcc contracts a * b + c to an FMA by default: the arithmetic below is written with operators under this file's
// pragma, everything is evaluated as written, one rounding per operation (as cb_resize.hip).
#pragma clang fp contract(off)

namespace {

#define CBW_MAXEXT (1 << 15)
#define CBW_LIMIT 1048576.f      // 2^20 px

typedef _Float16 cbw_half2 __attribute__((ext_vector_type(2)));

// KIND: CB_WARP_NEAREST, CB_WARP_BILINEAR, CB_WARP_BICUBIC
template <int KIND>
struct cbw_kind {
    static constexpr int taps = KIND == CB_WARP_NEAREST ? 1 : (KIND == CB_WARP_BILINEAR ? 2 : 4);
};

struct cbw_geo {
    int Hi, Wi, Ho, Wo, padding, align, flow;
};

// the coordinate pair (x, y) of output pixel p = oy Wo + ox, exactly as f32
__device__ __forceinline__ void cbw_load_pair(const float* c, long p, long HWo, int flow, float& x, float& y) {
    if (flow) {
        x = c[p];
        y = c[HWo + p];
    } else {
        const float2 v = *(const float2*)(c + 2 * p);
        x = v.x;
        y = v.y;
    }
}
__device__ __forceinline__ void cbw_load_pair(const cb_half* c, long p, long HWo, int flow, float& x, float& y) {
    if (flow) {
        x = (float)c[p];
        y = (float)c[HWo + p];
    } else {
        const cbw_half2 v = *(const cbw_half2*)(c + 2 * p);
        x = (float)v.x;
        y = (float)v.y;
    }
}

__device__ __forceinline__ float cbw_clip(float s, int n) {
    const float hi = (float)(n - 1);
    return s < 0.f ? 0.f : (s > hi ? hi : s);
}

// the header's padding of a coordinate (nearest and bilinear)
__device__ __forceinline__ float cbw_pad_coord(float s, int n, int padding, int align) {
    if (padding == CB_WARP_BORDER) return cbw_clip(s, n);
    if (padding == CB_WARP_REFLECTION) {
        const float lo = align ? 0.f : -0.5f, span = align ? (float)(n - 1) : (float)n;
        if (span == 0.f) return 0.f;
        const float a = fabsf(s - lo), e = fmodf(a, span);
        // a - e is span times an integer below 2^21, exactly: the correctly rounded quotient is that integer
        const int k = (int)__fdiv_rn(a - e, span);
        float r = (k & 1) ? span - e : e;
        r = r + lo;
        return cbw_clip(r, n);
    }
    return s;
}

// ... and of a bicubic tap index (|i| <= 2^20 + 2)
__device__ __forceinline__ int cbw_pad_index(int i, int n, int padding, int align) {
    if (padding == CB_WARP_BORDER) return min(max(i, 0), n - 1);
    if (padding == CB_WARP_REFLECTION) {
        if (n == 1) return 0;
        if (align) {
            const int period = 2 * (n - 1), m = abs(i) % period;
            return m > n - 1 ? period - m : m;
        }
        const int m = (i < 0 ? -1 - i : i) % (2 * n);
        return m >= n ? 2 * n - 1 - m : m;
    }
    return i;
}

// the cubic convolution weights of the resize section, A = -0.75
__device__ __forceinline__ float cbw_w_far(float s) {
    float m = -0.75f * s;
    m = m - -3.75f;
    m = m * s;
    m = m + -6.f;
    m = m * s;
    return m - -3.f;
}
__device__ __forceinline__ float cbw_w_near(float t) {
    float m = 1.25f * t;
    m = m - 2.25f;
    m = m * t;
    m = m * t;
    return m + 1.f;
}

// One axis of n input pixels: the source coordinate from the pixel's coordinate v (grid: normalised; flow: the
// displacement of output coordinate o), then the KIND's taps -- an index in the map, or -1 -- and weights.
template <int KIND>
__device__ __forceinline__ void cbw_axis(float v, int o, int n, const cbw_geo& g, int (&tap)[4], float (&w)[4]) {
    float s;
    if (g.flow) {
        s = (float)o + v;
    } else if (g.align) {
        s = v + 1.f;
        s = s * 0.5f;
        s = s * (float)(n - 1);
    } else {
        s = v + 1.f;
        s = s * (float)n;
        s = s - 1.f;
        s = s * 0.5f;
    }
    s = !(s > -CBW_LIMIT) ? -CBW_LIMIT : (s > CBW_LIMIT ? CBW_LIMIT : s);
    if (KIND != CB_WARP_BICUBIC) s = cbw_pad_coord(s, n, g.padding, g.align);
    if (KIND == CB_WARP_NEAREST) {
        tap[0] = (int)rintf(s);
    } else if (KIND == CB_WARP_BILINEAR) {
        const float f = floorf(s);
        tap[0] = (int)f;
        tap[1] = tap[0] + 1;
        w[0] = (f + 1.f) - s;
        w[1] = s - f;
    } else {
        const float f = floorf(s), t = s - f;
        const int i0 = (int)f;
#pragma unroll
        for (int k = 0; k < 4; ++k) tap[k] = cbw_pad_index(i0 - 1 + k, n, g.padding, g.align);
        w[0] = cbw_w_far(t + 1.f);
        w[1] = cbw_w_near(t);
        w[2] = cbw_w_near(1.f - t);
        w[3] = cbw_w_far(2.f - t);
    }
#pragma unroll
    for (int k = 0; k < cbw_kind<KIND>::taps; ++k)
        if ((unsigned)tap[k] >= (unsigned)n) tap[k] = -1;      // (no address is ever formed from it)
}

// in [C, Hi, Wi], coords [Ho, Wo, 2] or [2, Ho, Wo], out [C, Ho, Wo].  inMask: the input's change mask of this frame
// over the INPUT map (its own, or the working mask its list went into); coordMask: the coordinates' mask over the
// output map, or NULL (a list is in `bits` already); all: every output pixel is listed, neither mask is read.
template <typename T, typename CT, int KIND>
__global__ __launch_bounds__(256) void cbw_warp_kernel(const T* __restrict__ in, const CT* __restrict__ coords,
                                                      T* __restrict__ out,
                                                      const unsigned long long* __restrict__ inMask,
                                                      const unsigned long long* __restrict__ coordMask, int all,
                                                      unsigned long long* bits,
                                                      unsigned long long* __restrict__ maskCopy, long words, int C,
                                                      cbw_geo g, int wprI, int wprO) {
    constexpr int TAPS = cbw_kind<KIND>::taps;
    // the four waves' ballots, used in turn: a region is written again only behind the barrier of the word after it
    __shared__ unsigned long long foot[2][4];
    // a word's records, [field][pixel]: offsets (or -1) and weights
    __shared__ int recI[8][64];
    __shared__ float recF[8][64];
    const long HWi = (long)g.Hi * g.Wi, HWo = (long)g.Ho * g.Wo;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int tx[4], ty[4];      // the taps of this lane's pixel: made by makeWord, read by the unit
    float wx[4], wy[4];
    unsigned turn = 0;
    cb_walk_word_units(
        bits, maskCopy, words, g.Wo, wprO, all,
        [&](long w, int oy, int tile) {
            const int ox = tile * 64 + lane;
#pragma unroll
            for (int k = 0; k < 4; ++k) tx[k] = ty[k] = -1, wx[k] = wy[k] = 0.f;
            if (ox < g.Wo) {
                float cx, cy;
                cbw_load_pair(coords, (long)oy * g.Wo + ox, HWo, g.flow, cx, cy);
                cbw_axis<KIND>(cx, ox, g.Wi, g, tx, wx);
                cbw_axis<KIND>(cy, oy, g.Hi, g, ty, wy);
            }
            if (all) return 0ull;
            unsigned long long word = coordMask ? coordMask[w] : 0ull;
            if (inMask) {      // (uniform over the workgroup, and so is the barrier)
                bool hit = false;
#pragma unroll
                for (int k = 0; k < TAPS; ++k) {
                    if (k != wave || ty[k] < 0) continue;      // wave k tests tap row k
                    const unsigned long long* row = inMask + (long)ty[k] * wprI;
                    unsigned long long m = 0ull;
                    int have = -1;
#pragma unroll
                    for (int j = 0; j < TAPS; ++j) {
                        if (tx[j] < 0) continue;
                        if ((tx[j] >> 6) != have) {
                            have = tx[j] >> 6;
                            m = row[have];
                        }
                        hit |= ((m >> (tx[j] & 63)) & 1ull) != 0;
                    }
                }
                const unsigned long long mine = __ballot(hit);
                unsigned long long* f = foot[turn++ & 1u];
                if (lane == 0) f[wave] = mine;
                __syncthreads();
                word |= f[0] | f[1] | f[2] | f[3];
            }
            return word;
        },
        [&](unsigned long long word, int oy, int tile) {
            if ((word >> lane) & 1ull) {      // each listed pixel's record, once: the fields dealt over the waves
                if (KIND == CB_WARP_NEAREST) {
                    if (wave == 0) recI[0][lane] = (ty[0] >= 0 && tx[0] >= 0) ? ty[0] * g.Wi + tx[0] : -1;
                } else if (KIND == CB_WARP_BILINEAR) {
#pragma unroll
                    for (int k = 0; k < 2; ++k)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if (wave == 0) recI[2 * k + j][lane] = (ty[k] >= 0 && tx[j] >= 0) ? ty[k] * g.Wi + tx[j] : -1;
                            if (wave == 1) recF[2 * k + j][lane] = wx[j] * wy[k];
                        }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (wave == 0) recI[k][lane] = tx[k];
                        if (wave == 1) recI[4 + k][lane] = ty[k] >= 0 ? ty[k] * g.Wi : -1;
                        if (wave == 2) recF[k][lane] = wx[k];
                        if (wave == 3) recF[4 + k][lane] = wy[k];
                    }
                }
            }
            __syncthreads();
            const int n = __popcll(word), total = n * C;
            for (int e = threadIdx.x; e < total; e += 256) {
                const int c = e / n, i = e - c * n;
                const int bit = n == 64 ? i : cb_select_bit(word, i);
                const T* src = in + (long)c * HWi;
                T res;
                if (KIND == CB_WARP_NEAREST) {
                    const int o = recI[0][bit];
                    res = o >= 0 ? src[o] : (T)0.f;      // (a copy: bit for bit)
                } else if (KIND == CB_WARP_BILINEAR) {
                    float acc = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int o = recI[k][bit];
                        if (o >= 0) {
                            const float term = recF[k][bit] * cb_load_f32(src + o);
                            acc = acc + term;
                        }
                    }
                    res = (T)acc;
                } else {
                    float acc = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int oyk = recI[4 + k][bit];
                        float r = 0.f;
                        if (oyk >= 0) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int oxj = recI[j][bit];
                                if (oxj >= 0) {
                                    const float term = recF[j][bit] * cb_load_f32(src + oyk + oxj);
                                    r = r + term;
                                }
                            }
                        }
                        const float term = recF[4 + k][bit] * r;
                        acc = acc + term;
                    }
                    res = (T)acc;
                }
                out[(long)c * HWo + (long)oy * g.Wo + tile * 64 + bit] = res;
            }
            __syncthreads();      // every item has read the records before the next word's are written
        });
}

// behind a frame whose input came as a list: zero to the words of the input working mask that the list named (plain
// stores of one value: entries that share a word do not matter)
__global__ __launch_bounds__(256) void cbw_clear_list_kernel(const int32_t* __restrict__ list, int nHost,
                                                            const int32_t* __restrict__ countDev, int H, int W, int wpr,
                                                            unsigned long long* __restrict__ inBits) {
    const int N = countDev ? min(*countDev, nHost) : nHost;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        const int pos = list[i];
        if ((unsigned)pos >= (unsigned)(H * W)) continue;      // (an out-of-map entry set no bit)
        const int y = pos / W, x = pos - y * W;
        inBits[(long)y * wpr + (x >> 6)] = 0ull;
    }
}

template <typename T, typename CT>
void cbw_launch(const void* in, const void* coords, void* out, const uint64_t* inMask, const uint64_t* coordMask, int all,
                uint64_t* bits, uint64_t* maskCopy, int C, const cbw_geo& g, int mode, hipStream_t s) {
    const int wprO = (g.Wo + 63) / 64, wprI = (g.Wi + 63) / 64;
    const long words = (long)g.Ho * wprO;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBW_GO(KIND)                                                                                                    \
    if (mode == KIND)                                                                                                   \
    hipLaunchKernelGGL((cbw_warp_kernel<T, CT, KIND>), grid, block, 0, s, (const T*)in, (const CT*)coords, (T*)out,     \
                       (const unsigned long long*)inMask, (const unsigned long long*)coordMask, all,                    \
                       (unsigned long long*)bits, (unsigned long long*)maskCopy, words, C, g, wprI, wprO)
    CBW_GO(CB_WARP_NEAREST);
    CBW_GO(CB_WARP_BILINEAR);
    CBW_GO(CB_WARP_BICUBIC);
#undef CBW_GO
}

inline bool cbw_extent_ok(int n) { return n >= 1 && n < CBW_MAXEXT; }

}  // namespace

int cbinfer_warp_supported(const cbWarp* w, int Hi, int Wi) {
    if (!w) return 0;
    return cbw_extent_ok(Hi) && cbw_extent_ok(Wi) && cbw_extent_ok(w->Ho) && cbw_extent_ok(w->Wo) &&
           w->mode >= CB_WARP_NEAREST && w->mode <= CB_WARP_BICUBIC && w->padding >= CB_WARP_ZEROS &&
           w->padding <= CB_WARP_REFLECTION && (w->alignCorners == 0 || w->alignCorners == 1) &&
           (w->coordKind == CB_WARP_GRID || w->coordKind == CB_WARP_FLOW) &&
           (w->coordDtype == CB_F32 || w->coordDtype == CB_F16);
}

int cbinfer_cbwarp_forward(const void* input, const void* coords, void* outputState, const uint64_t* inputMask,
                           const int32_t* inputList, int inputCap, const int32_t* inputCount, const uint64_t* coordMask,
                           const int32_t* coordList, int coordCap, const int32_t* coordCount, uint64_t* inBits,
                           uint64_t* bits, uint64_t* maskCopy, int C, int Hi, int Wi, const cbWarp* warp, int dtype,
                           cbStream_t stream) {
    // (every argument is checked before the first launch)
    CB_REQUIRE(input && coords && outputState && outputState != input && outputState != coords && C >= 1);
    CB_REQUIRE(inBits && bits && maskCopy && inBits != bits && inBits != maskCopy && bits != maskCopy);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16);
    CB_REQUIRE(cbinfer_warp_supported(warp, Hi, Wi));
    CB_REQUIRE(inputCap >= 0 && !(inputMask && inputList) && (inputList || !inputCount));
    CB_REQUIRE(coordCap >= 0 && !(coordMask && coordList) && (coordList || !coordCount));
    CB_REQUIRE(inputMask != inBits && inputMask != bits && inputMask != maskCopy);
    CB_REQUIRE(coordMask != inBits && coordMask != bits && coordMask != maskCopy);
    // (the kernel numbers a word's items with an int)
    CB_REQUIRE((long)C * 64 < (1l << 31));
    const cbw_geo g = {Hi, Wi, warp->Ho, warp->Wo, warp->padding, warp->alignCorners, warp->coordKind == CB_WARP_FLOW};
    const hipStream_t s = (hipStream_t)stream;
    // an operand with neither mask nor list lists every output pixel: the other's changes are not needed then
    const int all = (!inputMask && !inputList) || (!coordMask && !coordList);
    const bool inList = !all && inputList && inputCap > 0;
    if (inList) {
        const int st = cb_list_to_bits(inputList, inputCap, inputCount, Hi, Wi, inBits, stream);
        if (st != CB_OK) return st;
    }
    if (!all && coordList) {
        const int st = cb_list_to_bits(coordList, coordCap, coordCount, g.Ho, g.Wo, bits, stream);
        if (st != CB_OK) return st;
    }
    const uint64_t* inMask = all ? nullptr : (inputMask ? inputMask : (inList ? inBits : nullptr));
    cb_dispatch_dtype(dtype, [&](auto t) {
        cb_dispatch_dtype(warp->coordDtype, [&](auto ct) {
            cbw_launch<decltype(t), decltype(ct)>(input, coords, outputState, inMask, all ? nullptr : coordMask, all, bits,
                                                  maskCopy, C, g, warp->mode, s);
        });
    });
    int st = cb_launch_status();
    if (st != CB_OK || !inList) return st;
    long blocks = ((long)inputCap + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(cbw_clear_list_kernel, dim3((unsigned)blocks), dim3(256), 0, s, inputList, inputCap, inputCount, Hi,
                       Wi, (Wi + 63) / 64, (unsigned long long*)inBits);
    return cb_launch_status();
}
