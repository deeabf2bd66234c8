// Change-based peak suppression (non-maximum suppression by a k x k or cross-shaped neighbourhood, with an optional
// floor) and the ordered peak list on gfx950.  The reference's pose detector copies its full-resolution
// heat maps to the host and searches the peaks there; torch has no module for the operator (CenterNet-type heads write
// heat * (max_pool2d(heat, 3, 1, 1) == heat)).  Contracts of the entry points in include/cbinfer_hip.h.  Whether a
// pixel is a peak depends on its neighbourhood alone, and every producer of this library leaves the pixels outside its
// change list bit for bit as they were: recomputing at the k x k / stride-1 FOOTPRINT of the operand's changes gives the
// dense result exactly, without a threshold.  A frame is
//   for an operand in LIST form, one launch in front: the list's footprint ORed into the zeroed working mask
//              (cbinfer_pool_footprint of cb_pool2d.hip with the window as a stride-1 max pool);
//   one launch, the word-level walk of cb_maskwalk.h (cb_walk_word_units): an operand in mask form has its footprint
//              gathered word by word inside the walk.  The unit of work is (non-empty mask word, channel): one wave a
//              unit, the four waves of the workgroup stride over the channels -- several channels a round, their loads
//              requested together --, lane <-> column 64 tile + lane.
//   for the peak list, three more launches (cbinfer_peaks_list): popcounts per (channel, row), an exclusive scan in ONE
//              workgroup, the entries.
// No LDS in the suppression kernel, no atomics in any kernel of this file, no workgroup waits for another one, no host
// sync, memset, allocation or inline assembly; all stores are plain vector stores.
#include <math.h>

#include "cb_maskwalk.h"

namespace {

// The maximum under which a NaN wins and stays (torch's max_pool2d rule): NaN if either is one, else the larger.
__device__ __forceinline__ float cbk_max(float m, float t) { return (t > m || t != t) ? t : m; }

// One value of the map as f32 (exact), -inf -- the padding of a max pool -- where (yy, xx) lies outside it.  The load is
// unconditional, from the clamped position: the loads of a unit are requested together.
template <typename T>
__device__ __forceinline__ float cbk_at(const T* __restrict__ src, int yy, int xx, int H, int W) {
    const float v = cb_load_f32(src + (long)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1));
    return ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? v : -INFINITY;
}

// The footprint word (y, tile) of an operand's change mask under the (2 rH + 1) x (2 rW + 1) / stride-1 window: the OR of
// the rows y - rH .. y + rH of the word and its two neighbours, dilated by rW along the row.  Scalar: every thread
// computes the same word from the same addresses.  (Not cut to the row: the walk does that.)
__device__ __forceinline__ unsigned long long cbk_footprint_word(const unsigned long long* __restrict__ mask, int y,
                                                                  int tile, int H, int wpr, int rH, int rW) {
    unsigned long long m = 0ull, l = 0ull, r = 0ull;
    for (int yy = max(y - rH, 0); yy <= min(y + rH, H - 1); ++yy) {
        const unsigned long long* row = mask + (long)yy * wpr;
        m |= row[tile];
        if (tile > 0) l |= row[tile - 1];
        if (tile + 1 < wpr) r |= row[tile + 1];
    }
    unsigned long long d = m;
    for (int k = 1; k <= rW; ++k) d |= (m << k) | (m >> k) | (l >> (64 - k)) | (r << (64 - k));
    return d;
}

// x, out [C, H, W]; peakBits [C][words].  mask: the OPERAND's change mask of this frame, or NULL; all: every pixel is
// listed.  An operand in list form has its footprint in `bits` already.  RH: the vertical radius; CROSS (RH == 1): the
// centre and its four neighbours.
template <typename T, int RH, bool CROSS>
__global__ __launch_bounds__(256) void cbk_peaks_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                       unsigned long long* __restrict__ peakBits,
                                                       const unsigned long long* __restrict__ mask, int all,
                                                       unsigned long long* bits, unsigned long long* __restrict__ maskCopy,
                                                       long words, int C, int H, int W, int wpr, int rW, int hasFloor,
                                                       float floorValue) {
    const long HW = (long)H * W;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cb_walk_word_units(
        bits, maskCopy, words, W, wpr, all,
        [&](long, int y, int tile) { return mask ? cbk_footprint_word(mask, y, tile, H, wpr, RH, rW) : 0ull; },
        [&](unsigned long long word, int y, int tile) {
            const int col = tile * 64 + lane;
            // the halo: lane j < rW owns column 64 tile - rW + j, lane rW <= j < 2 rW column 64 tile + 64 + j - rW
            // (every other lane loads its own column again)
            const int hcol = lane < rW ? tile * 64 - rW + lane : lane < 2 * rW ? tile * 64 + 64 + lane - rW : col;
            const bool listed = (word >> lane) & 1ull;
            const unsigned long long valid = cb_valid_mask(W, tile);
            const long w = (long)y * wpr + tile;
            // A wave takes NB of its channels (wave, wave + 4, ...) per round: all their loads are requested before the
            // first value is used.  A slot beyond C loads channel C - 1 again and stores nothing (uniform over the wave).
            constexpr int NB = RH == 1 ? 4 : 2, ROWS = 2 * RH + 1;
            for (int c0 = wave; c0 < C; c0 += 4 * NB) {
                T own[NB];
                float a[NB][ROWS], h[NB][ROWS];
                unsigned long long old[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int c = min(c0 + 4 * u, C - 1);
                    const T* src = x + (long)c * HW;
                    // (the centre's own bits: what a kept pixel stores)
                    own[u] = src[(long)y * W + min(col, W - 1)];
                    // the rows of the lane's own column and of its halo column: 2 (2 RH + 1) loads a lane, coalesced
                    // along the row.  CROSS: only the centre row spreads sideways.
#pragma unroll
                    for (int d = 0; d < ROWS; ++d) {
                        a[u][d] = cbk_at(src, y + d - RH, col, H, W);
                        h[u][d] = (CROSS && d != RH) ? -INFINITY : cbk_at(src, y + d - RH, hcol, H, W);
                    }
                    old[u] = lane == 0 ? peakBits[(long)c * words + w] : 0ull;
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int c = c0 + 4 * u;
                    float best = a[u][0], halo = h[u][0];
#pragma unroll
                    for (int d = 1; d < ROWS; ++d) {
                        best = cbk_max(best, a[u][d]);
                        halo = cbk_max(halo, h[u][d]);
                    }
                    const float side = CROSS ? a[u][RH] : best;      // (what the lane shows the lanes beside it)
                    // the neighbours at distance k along the row, from the lanes beside or from the halo lanes
                    for (int k = 1; k <= rW; ++k) {
#pragma unroll
                        for (int sgn = -1; sgn <= 1; sgn += 2) {
                            const int from = lane + sgn * k;
                            const float inWord = __shfl(side, from & 63);
                            const float beyond = __shfl(halo, from < 0 ? rW + from : rW + (from & 63));
                            best = cbk_max(best, (unsigned)from < 64u ? inWord : beyond);
                        }
                    }
                    const float v = a[u][RH];
                    // (v >= best: v is the neighbourhood's maximum; false if there is a NaN in it, v included)
                    const bool keep = listed && v >= best && (!hasFloor || v >= floorValue);
                    const unsigned long long kept = __ballot(keep);
                    if (c < C) {
                        if (listed) out[(long)c * HW + (long)y * W + col] = keep ? own[u] : (T)0.f;
                        if (lane == 0) peakBits[(long)c * words + w] = (old[u] & ~word & valid) | kept;
                    }
                }
            }
        });
}

template <typename T>
void cbk_launch(const void* x, void* out, uint64_t* peakBits, const uint64_t* mask, int all, uint64_t* bits,
                uint64_t* maskCopy, int C, int H, int W, const cbPeaks& p, hipStream_t s) {
    const int wpr = (W + 63) / 64;
    const long words = (long)H * wpr;
    const dim3 grid(cb_walk_grid(words)), block(256);
#define CBK_GO(RH, CROSS)                                                                                             \
    hipLaunchKernelGGL((cbk_peaks_kernel<T, RH, CROSS>), grid, block, 0, s, (const T*)x, (T*)out,                    \
                       (unsigned long long*)peakBits, (const unsigned long long*)mask, all, (unsigned long long*)bits, \
                       (unsigned long long*)maskCopy, words, C, H, W, wpr, p.kW / 2, p.hasFloor, p.floor)
    if (p.cross)
        CBK_GO(1, true);
    else if (p.kH == 3)
        CBK_GO(1, false);
    else if (p.kH == 5)
        CBK_GO(2, false);
    else
        CBK_GO(3, false);
#undef CBK_GO
}

// ---------------------------------------------------------------------------------------------------- the peak list
// Launch 1: work[c H + y] = the peaks of row y of channel c; work[C H] = 0.  One thread a row.  (Both list kernels
// cut a word to the pixels of the row: a caller's stale padding bit is no peak and addresses nothing.)
__global__ __launch_bounds__(256) void cbk_row_counts_kernel(const unsigned long long* __restrict__ peakBits,
                                                            int32_t* __restrict__ work, int rows, int W, int wpr) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    int n = 0;
    if (r < rows)
        for (int t = 0; t < wpr; ++t) n += __popcll(peakBits[(long)r * wpr + t] & cb_valid_mask(W, t));
    work[r] = n;
}

// Launch 2: the exclusive scan of work[0 .. rows] in place, by ONE workgroup of 1024 threads: a thread sums a run of
// `per` neighbouring entries, the sums are scanned in LDS (ten doubling steps), the thread writes its run's prefixes.
// work[rows] becomes the number of peaks: `count`; the prefix in front of a channel's first row: channelStart[c].
__global__ __launch_bounds__(1024) void cbk_scan_kernel(int32_t* __restrict__ work, int32_t* __restrict__ count,
                                                       int32_t* __restrict__ channelStart, int rows, int H, int per) {
    __shared__ int sums[2][1024];
    const int t = threadIdx.x;
    const long first = (long)t * per;
    int sum = 0;
    for (int i = 0; i < per; ++i)
        if (first + i <= rows) sum += work[first + i];
    int turn = 0;
    sums[0][t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        sums[turn ^ 1][t] = sums[turn][t] + (t >= off ? sums[turn][t - off] : 0);
        turn ^= 1;
        __syncthreads();
    }
    int run = sums[turn][t] - sum;      // (exclusive)
    for (int i = 0; i < per; ++i) {
        const long r = first + i;
        if (r > rows) break;
        const int n = work[r];
        work[r] = run;
        if (r % H == 0) channelStart[r / H] = run;      // (r == rows: channelStart[C], the total)
        if (r == rows) *count = run;
        run += n;
    }
}

// Launch 3: the entries.  One thread a word of peakBits; the word's first entry stands at its row's prefix plus the
// peaks of the row's earlier words.  Entry e < capN: (c, y, x) and the score x[c, y, x]; nothing is written beyond capN.
template <typename T>
__global__ __launch_bounds__(256) void cbk_entries_kernel(const T* __restrict__ x,
                                                         const unsigned long long* __restrict__ peakBits,
                                                         const int32_t* __restrict__ work, int32_t* __restrict__ entries,
                                                         T* __restrict__ scores, int capN, long total, int H, int W,
                                                         int wpr) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long row = i / wpr;
    const int tile = (int)(i - row * wpr);
    unsigned long long word = peakBits[i] & cb_valid_mask(W, tile);
    if (word == 0ull) return;
    const int c = (int)(row / H), y = (int)(row - (long)c * H);
    int e = work[row];
    for (int t = 0; t < tile; ++t) e += __popcll(peakBits[row * wpr + t]);      // (full words: t < tile)
    for (; word != 0ull && e < capN; word &= word - 1ull, ++e) {
        const int px = tile * 64 + __builtin_ctzll(word);
        entries[3l * e] = c;
        entries[3l * e + 1] = y;
        entries[3l * e + 2] = px;
        scores[e] = x[row * W + px];
    }
}

// what the suppression entry points ask of the tensors, the module's masks and the window
int cbk_args(const void* x, const void* out, const uint64_t* peakBits, const uint64_t* mask, const uint64_t* bits,
             const uint64_t* maskCopy, int C, int H, int W, const cbPeaks* p, int dtype) {
    CB_REQUIRE(x && out && x != out && peakBits && bits && maskCopy && p && bits != maskCopy && mask != bits &&
               mask != maskCopy && peakBits != bits && peakBits != maskCopy && peakBits != mask);
    CB_REQUIRE(C >= 1 && H >= 1 && W >= 1 && (dtype == CB_F32 || dtype == CB_F16));
    if (!cbinfer_peaks_supported(p)) return CB_ERR_UNSUPPORTED;
    // (a list addresses a pixel with an int32, the walk numbers a word's rows with one)
    if ((long)H * W >= (1l << 31) || (long)C * 64 >= (1l << 31)) return CB_ERR_UNSUPPORTED;
    return CB_OK;
}

}  // namespace

int cbinfer_peaks_supported(const cbPeaks* p) {
    if (!p) return 0;
    const auto window = [](int k) { return k == 3 || k == 5 || k == 7; };
    if (!window(p->kH) || !window(p->kW)) return 0;
    if (p->cross != 0 && (p->cross != 1 || p->kH != 3 || p->kW != 3)) return 0;
    if (p->hasFloor != 0 && (p->hasFloor != 1 || !__builtin_isfinite(p->floor))) return 0;
    return 1;
}

int cbinfer_peaks_changed(const void* x, void* out, uint64_t* peakBits, const uint64_t* mask, int all, uint64_t* bits,
                          uint64_t* maskCopy, int C, int H, int W, const cbPeaks* peaks, int dtype, cbStream_t stream) {
    const int st = cbk_args(x, out, peakBits, mask, bits, maskCopy, C, H, W, peaks, dtype);
    if (st != CB_OK) return st;
    cb_dispatch_dtype(dtype, [&](auto t) {
        cbk_launch<decltype(t)>(x, out, peakBits, mask, all, bits, maskCopy, C, H, W, *peaks, (hipStream_t)stream);
    });
    return cb_launch_status();
}

int cbinfer_cbpeaks_forward(const void* x, void* outputState, uint64_t* peakBits, const uint64_t* mask,
                            const int32_t* list, int capN, const int32_t* countDev, uint64_t* bits, uint64_t* maskCopy,
                            int C, int H, int W, const cbPeaks* peaks, int dtype, cbStream_t stream) {
    // (every argument is checked before the first launch)
    int st = cbk_args(x, outputState, peakBits, mask, bits, maskCopy, C, H, W, peaks, dtype);
    if (st != CB_OK) return st;
    CB_REQUIRE(capN >= 0 && !(mask && list) && (list || !countDev));
    if (list) {
        const cbPool window = {peaks->kH, peaks->kW, 1, 1, peaks->kH / 2, peaks->kW / 2, 0, CB_POOL_MAX};
        st = cbinfer_pool_footprint(list, capN, countDev, nullptr, H, W, &window, bits, stream);
        if (st != CB_OK) return st;
    }
    return cbinfer_peaks_changed(x, outputState, peakBits, mask, !mask && !list, bits, maskCopy, C, H, W, peaks, dtype,
                                 stream);
}

int cbinfer_peaks_list(const void* x, const uint64_t* peakBits, int32_t* work, int32_t* entries, void* scores, int capN,
                       int32_t* count, int32_t* channelStart, int C, int H, int W, int dtype, cbStream_t stream) {
    CB_REQUIRE(x && peakBits && work && count && channelStart && capN >= 0 && (capN == 0 || (entries && scores)));
    CB_REQUIRE(C >= 1 && H >= 1 && W >= 1 && (dtype == CB_F32 || dtype == CB_F16));
    const int wpr = (W + 63) / 64;
    // (an entry's position, a row's number and a word's are int32 on the device: every pixel may be a peak)
    if ((long)C * H * W >= (1l << 31) || (long)C * H * wpr >= (1l << 31)) return CB_ERR_UNSUPPORTED;
    const int rows = C * H;
    const long total = (long)rows * wpr;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cbk_row_counts_kernel, dim3((unsigned)(rows / 256 + 1)), dim3(256), 0, s,
                       (const unsigned long long*)peakBits, work, rows, W, wpr);
    int st = cb_launch_status();
    if (st != CB_OK) return st;
    hipLaunchKernelGGL(cbk_scan_kernel, dim3(1), dim3(1024), 0, s, work, count, channelStart, rows, H,
                       rows / 1024 + 1);
    st = cb_launch_status();
    if (st != CB_OK) return st;
    cb_dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((cbk_entries_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const T*)x,
                           (const unsigned long long*)peakBits, (const int32_t*)work, entries, (T*)scores, capN, total, H,
                           W, wpr);
    });
    return cb_launch_status();
}
