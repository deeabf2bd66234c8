// Change-based grouped convolution for gfx950 (1 < groups <= C): the 3x3 layer of ResNeXt / RegNet
// bottlenecks and ShuffleNet units.  G groups, Cg = C / G input and Kg = K / G output channels per group, a cbGeom as in
// cb_geomconv.hip.  Two launches per frame:
//   cbinfer_change_detection_geom  (cb_geomconv.hip, called as it is): change over ALL C channels, the exact footprint
//                      on the OUTPUT map, the frame-mask protocol;
//   cbgr_conv_kernel   derives the ascending list from that mask (or takes a list) and walks the items (tile of 64
//                      listed pixels, group, row tile): gathers the taps of the group's Cg channels through the
//                      group-relative k -> tap table, contracts them with the group's filter rows on the MFMA units
//                      (16x16 tiles: f16; f32 as bf16 triples, six products; or the exact f32 MFMA), adds the bias,
//                      applies the ReLU and scatters into the group's output planes.  No workspace and no split along k:
//                      the groups supply the parallelism.  No MFMA instruction holds rows of two groups.
// The mask -> list prologue and the tile's pixel lookup are cbg_conv_kernel's; they, the weight-row load and the 8-tap
// gather are written once in cb_geom_stage.h (DESIGN 5.22 on why the stage loop is not).
// Entry-point contracts: include/cbinfer_hip.h, "grouped convolution".
#include "cb_common.h"
#include "cb_geom_stage.h"

namespace {

int cbgr_rows(int Kg) { return Kg <= 16 ? 16 : Kg <= 32 ? 32 : 64; }
int cbgr_kgpad(int Kg) { const int r = cbgr_rows(Kg); return (Kg + r - 1) / r * r; }

// CB_OK if the channel counts divide into 2 or more groups and the geometry is within cbGeom's limits
int cbgr_shape_status(int C, int K, int groups, const cbGeom* geom) {
    int Ho, Wo;
    if (!geom || C < 1 || K < 1 || groups < 1) return CB_ERR_BADARG;
    // (a map large enough for every filter within the limits: only the geometry is judged)
    const int st = cbinfer_geom_out_size(64, 64, geom, &Ho, &Wo);
    if (st != CB_OK) return st;
    if (groups < 2 || C % groups || K % groups) return CB_ERR_UNSUPPORTED;
    return CB_OK;
}

// ... and the map: the tap table holds group-relative byte offsets in an int; the padded k's marker (dy = dx = -32768)
// is outside every map of fewer than 2^30 pixels (cb_geomconv.hip, weight preparation)
int cbgr_map_status(int C, int K, int groups, int Hi, int Wi, const cbGeom* geom, int dtype, int* Ho, int* Wo) {
    int st = cbgr_shape_status(C, K, groups, geom);
    if (st != CB_OK) return st;
    st = cbinfer_geom_out_size(Hi, Wi, geom, Ho, Wo);
    if (st != CB_OK) return st;
    if ((long)*Ho * *Wo >= (1l << 31)) return CB_ERR_BADARG;
    if ((long)(C / groups) * Hi * Wi * (dtype == CB_F16 ? 2 : 4) >= (1l << 31) || (long)Hi * Wi >= (1l << 30))
        return CB_ERR_UNSUPPORTED;
    return CB_OK;
}

// ---------------------------------------------------------------------------------------------
// weight preparation: W[G][KgP][CkkgP] in the tensors' element type (k contiguous, zero padded) from torch's
// [K][Cg][kH][kW], then the group-relative k -> tap table in cbg_prep_kernel's format (the same for every group).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cbgr_prep_kernel(const T* __restrict__ w, T* __restrict__ wp, int G, int Kg,
                                                       int Ckkg, int KgP, int CkkgP, int Hi, int Wi, cbGeom g) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x, total = (long)G * KgP * CkkgP;
    if (e < CkkgP) {
        // (a tap inside the map is within the group's Cg Hi Wi elements)
        const int k = (int)e, c = k / (g.kH * g.kW), r = k % (g.kH * g.kW);
        cbg_tab_entry<T>((int*)(wp + total), CkkgP, k, k >= Ckkg, c, (r / g.kW) * g.dH - g.pH, (r % g.kW) * g.dW - g.pW,
                         Hi, Wi);
    }
    if (e >= total) return;
    const int k = (int)(e % CkkgP), m = (int)(e / CkkgP % KgP), grp = (int)(e / ((long)CkkgP * KgP));
    wp[e] = (m < Kg && k < Ckkg) ? w[((long)grp * Kg + m) * Ckkg + k] : T(0);
}

// ---------------------------------------------------------------------------------------------
// contraction
// ---------------------------------------------------------------------------------------------
struct GroupConvParams {
    const void* W;       // prepared weights [G][KgP][CkkgP]
    const int* tab;      // tap table behind them
    const void* src;     // the map the gather reads [C, Hi, Wi]
    const void* bias;    // [K] or null
    void* out;           // [K, Ho, Wo]
    CbgListArgs L;
    int32_t* listOut;    // mask mode: the list and its length as a by-product
    int32_t* countOut;
    int G, Cg, Kg, KgP, CkkgP, Hi, Wi, Ho, Wo, sH, sW, relu;
};

// One 32-deep stage on ROWS filter rows x this wave's 16 pixel columns: acc[a] holds rows 16 a .. 16 a + 15 (C/D layout of
// the 16x16 MFMAs: pixel column lane & 15, row 4 (lane >> 4) + register).  Operand lanes: row / column lane & 15,
// k = 8 (lane >> 4) + j of a 32-deep instruction, k = lane >> 4 of the 4-deep f32 one.
template <int ARITH, int NACC>
__device__ __forceinline__ void cbgr_mfma_stage(const CbgStage<ARITH>& A, const CbgStage<ARITH>& B, int col, int lane,
                                                floatx4 (&acc)[NACC]) {
    const int r = lane & 15, kg = lane >> 4;
    if constexpr (ARITH == CB_F16) {
        const halfx8 b = *(const halfx8*)&B.v[col][kg * 8];
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const halfx8 w = *(const halfx8*)&A.v[a * 16 + r][kg * 8];
            acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, b, acc[a], 0, 0, 0);
        }
    } else if constexpr (ARITH == CB_F32S) {
        const int k0 = kg * 8;
        const bf16x8 bh = *(const bf16x8*)&B.v[0][col][k0], bm = *(const bf16x8*)&B.v[1][col][k0],
                     bl = *(const bf16x8*)&B.v[2][col][k0];
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const int ra = a * 16 + r;
            const bf16x8 ah = *(const bf16x8*)&A.v[0][ra][k0], am = *(const bf16x8*)&A.v[1][ra][k0],
                         al = *(const bf16x8*)&A.v[2][ra][k0];
            // the six cross products above 2^-24 of the product, smallest first (cbg_mfma_stage's order)
            floatx4 c = acc[a];
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
            acc[a] = c;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float b = B.v[col][4 * s + kg];
#pragma unroll
            for (int a = 0; a < NACC; ++a)
                acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(A.v[a * 16 + r][4 * s + kg], b, acc[a], 0, 0, 0);
        }
    }
}

// T: element type of the tensors; ARITH: CB_F16 (T = half), CB_F32S or CB_F32 (T = float); ROWS: filter rows of a group
// per item (16, 32 or 64).  256 threads = 4 waves; wave v owns pixel columns 16 v .. 16 v + 15 of the tile and ROWS / 16
// accumulators.  Per stage of 32 k the first 4 ROWS threads load 8 consecutive k of one filter row, and every thread gathers
// 8 consecutive k of one pixel -- a wave's k are uniform, so its taps come from the table by scalar loads --; the loads
// of stage s+1 are in flight while the MFMAs of stage s run (two LDS buffers, one barrier per stage).
template <typename T, int ARITH, int ROWS>
__global__ __launch_bounds__(256) void cbgr_conv_kernel(GroupConvParams p) {
    constexpr int NACC = ROWS / 16;
    __shared__ CbgStage<ARITH> sA[2], sB[2];
    __shared__ int sPre[257];
    __shared__ int sList[CBG_BN];
    __shared__ int sWave[4];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int NB = gridDim.x, HWo = p.Ho * p.Wo;

    // ---- the change list: from the frame mask (ascending by construction) or as given
    int N;
    const unsigned long long* cur = nullptr;
    const long words = p.L.maskWords;
    const int chunk = (int)((words + 255) / 256);
    if (p.L.frameMasks)
        N = cbg_list_from_mask(p.L.frameMasks, words, chunk, p.L.wpr, p.Wo, p.listOut, p.countOut, sPre, sWave, cur);
    else
        N = CBG_LIST_COUNT(p.L, HWo);
    if (N == 0) return;

    // ---- work items: (pixel tile, group, row tile), the row tile fastest
    const int tilesN = (N + CBG_BN - 1) / CBG_BN, rowTiles = p.KgP / ROWS, stages = p.CkkgP / CBG_BK;
    const long items = (long)tilesN * p.G * rowTiles;

    const int gn = t & 63, gk = wave * 8;      // gather: pixel row, first k of the stage
    const int am = t >> 2, ak = (t & 3) * 8;   // weights: filter row of the item, first k of the stage
    const int col = wave * 16 + (lane & 15);   // MFMA, epilogue: this lane's pixel column
    const long HWi = (long)p.Hi * p.Wi;

    for (long item = blockIdx.x; item < items; item += NB) {
        const int rt = (int)(item % rowTiles), grp = (int)(item / rowTiles % p.G), tn = (int)(item / ((long)rowTiles * p.G));
        __syncthreads();
        if (t < CBG_BN) {
            const int q = tn * CBG_BN + t;
            sList[t] = q < N ? cbg_list_entry(q, cur, sPre, words, chunk, p.L.wpr, p.Wo, p.L.list, HWo) : -1;
        }
        __syncthreads();

        const int pix = sList[gn];
        const int oy = pix < 0 ? 0 : pix / p.Wo, ox = pix < 0 ? 0 : pix % p.Wo;
        const int iy0 = oy * p.sH, ix0 = ox * p.sW;
        // (the group's Cg input planes: the base is added in 64 bits, the table's offsets are relative to it)
        const char* pbase = (const char*)((const T*)p.src + (long)grp * p.Cg * HWi + (long)iy0 * p.Wi + ix0);
        const T* wrow = (const T*)p.W + (((long)grp * p.KgP + (long)rt * ROWS + am) * p.CkkgP + ak);

        T ra[8], rb[8];
        auto load = [&](int s) {
            if (am < ROWS) cbg_load_wrow(ra, wrow + (long)s * CBG_BK);
            const int* tab = p.tab + s * CBG_BK + gk;
            CBG_GATHER8(T, rb, tab, p.CkkgP, pbase, pix, iy0, ix0, p.Hi, p.Wi);
        };
        auto put = [&](int b) {
            if (am < ROWS) sA[b].put(am, ak, ra);
            sB[b].put(gn, gk, rb);
        };

        floatx4 acc[NACC];
#pragma unroll
        for (int a = 0; a < NACC; ++a) acc[a] = floatx4{0.f, 0.f, 0.f, 0.f};
        // two LDS buffers, one barrier per stage: the loads of stage s+1 fly during the MFMAs of stage s and land in
        // the other buffer behind them (whose last readers passed the previous barrier)
        load(0);
        put(0);
        __syncthreads();
        for (int s = 0; s < stages; ++s) {
            const int cb = s & 1;
            if (s + 1 < stages) load(s + 1);
            cbgr_mfma_stage<ARITH, NACC>(sA[cb], sB[cb], col, lane, acc);
            if (s + 1 < stages) put(cb ^ 1);
            __syncthreads();
        }

        // ---- bias, ReLU, scatter: the group's real rows only
        const int opix = sList[col];
        if (opix >= 0) {
            T* out = (T*)p.out;
            const T* bias = (const T*)p.bias;
#pragma unroll
            for (int a = 0; a < NACC; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ml = rt * ROWS + a * 16 + (lane >> 4) * 4 + j;
                    if (ml < p.Kg) {
                        const int m = grp * p.Kg + ml;
                        float v = acc[a][j] + (bias ? (float)bias[m] : 0.f);
                        if (p.relu) v = v <= 0.f ? 0.f : v;
                        out[(long)m * HWo + opix] = (T)v;
                    }
                }
        }
    }
}

template <typename T, int ARITH>
void cbgr_launch_rows(const GroupConvParams& p, int rows, hipStream_t s) {
    dim3 grid(CBG_GRID), block(256);
    if (rows == 16)
        hipLaunchKernelGGL((cbgr_conv_kernel<T, ARITH, 16>), grid, block, 0, s, p);
    else if (rows == 32)
        hipLaunchKernelGGL((cbgr_conv_kernel<T, ARITH, 32>), grid, block, 0, s, p);
    else
        hipLaunchKernelGGL((cbgr_conv_kernel<T, ARITH, 64>), grid, block, 0, s, p);
}

int cbgr_launch_conv(const GroupConvParams& p, int dtype, hipStream_t s) {
    const int rows = cbgr_rows(p.Kg);
    cbg_dispatch_arith(dtype, [&](auto a) { cbgr_launch_rows<typename decltype(a)::T, decltype(a)::ARITH>(p, rows, s); });
    return cb_launch_status();
}

}  // namespace

extern "C" {

int cbinfer_groupconv_supported(int C, int K, int groups, const cbGeom* geom) {
    return cbgr_shape_status(C, K, groups, geom) == CB_OK;
}

long cbinfer_groupconv_prepared_weights_bytes(int K, int C, int groups, const cbGeom* geom, int dtype) {
    if (cbgr_shape_status(C, K, groups, geom) != CB_OK) return 0;
    const long KgP = cbgr_kgpad(K / groups), CkkgP = cbg_ckkpad(C / groups * geom->kH * geom->kW);
    return groups * KgP * CkkgP * (dtype == CB_F16 ? 2 : 4) + CkkgP * 8;
}

int cbinfer_groupconv_prep_weights(const void* weight, void* prepared, int K, int C, int groups, int Hi, int Wi,
                                   const cbGeom* geom, int dtype, cbStream_t stream) {
    CB_REQUIRE(weight && prepared && K > 0 && C > 0 && groups > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16 || dtype == CB_F32S);
    int Ho, Wo;
    const int st = cbgr_map_status(C, K, groups, Hi, Wi, geom, dtype, &Ho, &Wo);
    if (st != CB_OK) return st;
    const int Kg = K / groups, Ckkg = C / groups * geom->kH * geom->kW, KgP = cbgr_kgpad(Kg), CkkgP = cbg_ckkpad(Ckkg);
    dim3 grid(cb_div_up((long)groups * KgP * CkkgP, 256)), block(256);
    if (dtype == CB_F16)
        hipLaunchKernelGGL(cbgr_prep_kernel<cb_half>, grid, block, 0, (hipStream_t)stream, (const cb_half*)weight,
                           (cb_half*)prepared, groups, Kg, Ckkg, KgP, CkkgP, Hi, Wi, *geom);
    else
        hipLaunchKernelGGL(cbgr_prep_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)weight,
                           (float*)prepared, groups, Kg, Ckkg, KgP, CkkgP, Hi, Wi, *geom);
    return cb_launch_status();
}

int cbinfer_conv_changed_grouped(const void* input, const int32_t* changeList, int numChanges, const int32_t* countDev,
                                 uint64_t* frameMasks, int32_t* idxOut, int32_t* countOut, const void* prepared,
                                 const void* bias, void* output, int C, int Hi, int Wi, int K, int groups,
                                 const cbGeom* geom, int relu, int dtype, cbStream_t stream) {
    CB_REQUIRE(input && prepared && output && C > 0 && K > 0 && groups > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16 || dtype == CB_F32S);
    int Ho, Wo;
    const int st = cbgr_map_status(C, K, groups, Hi, Wi, geom, dtype, &Ho, &Wo);
    if (st != CB_OK) return st;
    GroupConvParams p = {};
    const int ls = cbg_list_args(p.L, changeList, numChanges, countDev, frameMasks, idxOut && countOut, Ho, Wo);
    if (ls != CB_OK || cbg_nothing_listed(p.L)) return ls;
    p.listOut = idxOut, p.countOut = countOut;
    p.G = groups, p.Cg = C / groups, p.Kg = K / groups;
    p.KgP = cbgr_kgpad(p.Kg), p.CkkgP = cbg_ckkpad(p.Cg * geom->kH * geom->kW);
    p.W = prepared;
    p.tab = (const int*)((const char*)prepared + (long)groups * p.KgP * p.CkkgP * (dtype == CB_F16 ? 2 : 4));
    p.src = input, p.bias = bias, p.out = output;
    p.Hi = Hi, p.Wi = Wi, p.Ho = Ho, p.Wo = Wo, p.sH = geom->sH, p.sW = geom->sW, p.relu = relu;
    return cbgr_launch_conv(p, dtype, (hipStream_t)stream);
}

int cbinfer_cbgroupconv2d_forward(const void* input, void* prevInput, void* prevOutput, uint64_t* frameMasks,
                                  int32_t* idx, int32_t* countDev, const void* prepared, const void* bias, int C, int Hi,
                                  int Wi, int K, int groups, const cbGeom* geom, float threshold, int feedbackLoop,
                                  int copyInput, int relu, int dtype, cbStream_t stream) {
    CB_REQUIRE(input && prevInput && prevOutput && frameMasks && idx && countDev && prepared);
    CB_REQUIRE(C > 0 && K > 0 && groups > 0);
    CB_REQUIRE(dtype == CB_F32 || dtype == CB_F16 || dtype == CB_F32S);
    int Ho, Wo;
    int st = cbgr_map_status(C, K, groups, Hi, Wi, geom, dtype, &Ho, &Wo);
    if (st != CB_OK) return st;
    if (Hi > 65535) return CB_ERR_UNSUPPORTED;      // (cbinfer_change_detection_geom's limit, before any launch)
    const CbgFrameMode fm = cbg_frame_mode(input, prevInput, feedbackLoop, copyInput, dtype);
    st = cbinfer_change_detection_geom(input, prevInput, frameMasks, C, Hi, Wi, geom, threshold, fm.update, fm.edt, stream);
    if (st != CB_OK) return st;
    return cbinfer_conv_changed_grouped(fm.src, nullptr, 0, nullptr, frameMasks, idx, countDev, prepared, bias, prevOutput, C,
                                        Hi, Wi, K, groups, geom, relu, dtype, stream);
}

}  // extern "C"
