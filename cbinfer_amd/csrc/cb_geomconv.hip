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

// ---------------------------------------------------------------------------------------------
// weight preparation: W[KP][CkkP] in the tensors' element type (k contiguous, zero padded), then the k -> tap table
// (cbg_tab_entry): tap (c, ky, kx) lies at dy = ky dH - pH, dx = kx dW - pW from the BASE pixel (oy sH, ox sW) of the
// input map.  The padded tail's marker needs a map of fewer than 2^30 pixels, which cbinfer_geom_prep_weights checks.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cbg_prep_kernel(const T* __restrict__ w, T* __restrict__ wp, int K, int Ckk,
                                                      int KP, int CkkP, int Hi, int Wi, cbGeom g) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < CkkP) {
        const int k = (int)e, c = k / (g.kH * g.kW), r = k % (g.kH * g.kW);
        cbg_tab_entry<T>((int*)(wp + (long)KP * CkkP), CkkP, k, k >= Ckk, c, (r / g.kW) * g.dH - g.pH,
                         (r % g.kW) * g.dW - g.pW, Hi, Wi);
    }
    if (e >= (long)KP * CkkP) return;
    const int k = (int)(e % CkkP), m = (int)(e / CkkP);
    wp[e] = (m < K && k < Ckk) ? w[(long)m * Ckk + k] : T(0);
}

// ---------------------------------------------------------------------------------------------
// detection: one workgroup = one 64-pixel row segment of the INPUT map x all channels (1 to 16 waves by the channel
// count; one coalesced row segment per wave load); the scan and the state refresh are cbg_detect_scan (cb_geom_stage.h).
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
    const int lane = threadIdx.x & 63, tx = blockIdx.x, y = blockIdx.y;
    const int x = tx * 64 + lane;
    const unsigned long long m = cbg_detect_scan(in, state, C, (long)Hi * Wi, (long)y * Wi + x, x < Wi, thf, update);
    if (m == 0) return;      // uniform over the workgroup
    if (threadIdx.x >> 6 != 0) return;      // (the footprint: wave 0)

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
    CbgListArgs L;
    int32_t* listOut;    // mask mode: the list and its length as a by-product
    int32_t* countOut;
    CbgWorkspace ws;
    int K, KP, CkkP, Hi, Wi, Ho, Wo, sH, sW, relu;
};

// The tile, its stages, the split along k and the epilogue: cb_geom_stage.h (CBG_TILE_STAGES, CBG_SPLITK_HANDOFF,
// CBG_TILE_STORE).  This kernel's own: the items (pixel tile, channel tile, k-slice) over ONE list, and the base input
// pixel (oy sH, ox sW) of an output pixel.
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
    const long words = p.L.maskWords;
    const int chunk = (int)((words + 255) / 256);
    if (p.L.frameMasks)
        N = cbg_list_from_mask(p.L.frameMasks, words, chunk, p.L.wpr, p.Wo, p.listOut, p.countOut, sPre, sWave, cur);
    else
        N = CBG_LIST_COUNT(p.L, HWo);
    if (N == 0) return;

    // ---- work items: (pixel tile, channel tile, k-slice)
    const int tilesN = (N + CBG_BN - 1) / CBG_BN, tilesM = p.KP / CBG_BM, stages = p.CkkP / CBG_BK;
    const int base = tilesN * tilesM;
    int SK = 1;
    if (p.ws.slabs && base < G) SK = max(1, min(min(G / base, CBG_SKMAX), stages));
    const int items = base * SK;      // (SK > 1: items <= G, one item and one slab per workgroup)
    const int gn = t & 63, gk = wave * 8;      // the thread's place in the tile (cb_geom_stage.h)
    const int am = t >> 2, ak = (t & 3) * 8;
    const int wm = wave & 1, wn = wave >> 1;
    const T* src = (const T*)p.src;

    for (int item = blockIdx.x; item < items; item += G) {
        const int slice = item % SK, tm = (item / SK) % tilesM, tn = item / (SK * tilesM);
        const int s0 = (int)((long)stages * slice / SK), s1 = (int)((long)stages * (slice + 1) / SK);
        __syncthreads();
        if (t < CBG_BN) {
            const int q = tn * CBG_BN + t;
            sList[t] = q < N ? cbg_list_entry(q, cur, sPre, words, chunk, p.L.wpr, p.Wo, p.L.list, HWo) : -1;
        }
        __syncthreads();

        const int pix = sList[gn];
        const int oy = pix < 0 ? 0 : pix / p.Wo, ox = pix < 0 ? 0 : pix % p.Wo;
        const int iy0 = oy * p.sH, ix0 = ox * p.sW;
        const char* pbase = (const char*)(src + (long)iy0 * p.Wi + ix0);
        const T* wrow = (const T*)p.W + ((long)tm * CBG_BM + am) * p.CkkP + ak;
        CBG_TILE_STAGES(acc, wrow, p.tab, p.CkkP, pbase, pix, iy0, ix0, p.Hi, p.Wi, s0, s1)
        if (SK > 1) CBG_SPLITK_HANDOFF(acc, p.ws.slabs, p.ws.tickets + (tn * tilesM + tm), item, slice, SK, sLast, continue)
        CBG_TILE_STORE(acc, sList, tm, p.bias, p.out, p.K, HWo, p.relu)
    }
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

long cbinfer_geom_workspace_bytes(void) { return cbg_workspace_bytes(); }

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
    return cbg_launch_detect(cbg_detect_kernel<float>, cbg_detect_kernel<cb_half>, input, state, frameMasks, C, Hi, Wi,
                             Ho, Wo, *geom, threshold, updateInputState, dtype, (hipStream_t)stream);
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
    const int ls = cbg_list_args(p.L, changeList, numChanges, countDev, frameMasks, idxOut && countOut, Ho, Wo);
    if (ls != CB_OK || cbg_nothing_listed(p.L)) return ls;
    p.listOut = idxOut, p.countOut = countOut;
    const int Ckk = C * geom->kH * geom->kW;
    p.KP = cbg_kpad(K), p.CkkP = cbg_ckkpad(Ckk);
    p.W = prepared;
    p.tab = (const int*)((const char*)prepared + (long)p.KP * p.CkkP * (dtype == CB_F16 ? 2 : 4));
    p.src = input, p.bias = bias, p.out = output;
    p.ws = cbg_workspace(workspace);
    p.K = K, p.Hi = Hi, p.Wi = Wi, p.Ho = Ho, p.Wo = Wo, p.sH = geom->sH, p.sW = geom->sW, p.relu = relu;
    cbg_dispatch_arith(dtype, [&](auto a) {
        hipLaunchKernelGGL((cbg_conv_kernel<typename decltype(a)::T, decltype(a)::ARITH>), dim3(CBG_GRID), dim3(256), 0,
                           (hipStream_t)stream, p);
    });
    return cb_launch_status();
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
    const CbgFrameMode fm = cbg_frame_mode(input, prevInput, feedbackLoop, copyInput, dtype);
    if (haveIndexes) {
        // propagated indexes address the input map: only where it is the output map do they mean what they mean for a
        // unit-geometry layer (no detection ran: the state copy is a copy)
        if (Ho != Hi || Wo != Wi) return CB_ERR_UNSUPPORTED;
        CB_REQUIRE(!feedbackLoop && capN >= 0 && capN <= Ho * Wo);
        if (fm.copyAll) {
            const hipError_t e = hipMemcpyAsync(prevInput, input, (size_t)C * Hi * Wi * (fm.edt == CB_F16 ? 2 : 4),
                                                hipMemcpyDeviceToDevice, (hipStream_t)stream);
            if (e != hipSuccess) return (int)e;
        }
        return cbinfer_conv_changed_geom(fm.src, idx, capN, countDev, nullptr, nullptr, nullptr, prepared, bias,
                                         prevOutput, C, Hi, Wi, K, geom, relu, workspace, dtype, stream);
    }
    CB_REQUIRE(frameMasks != nullptr);
    st = cbinfer_change_detection_geom(input, prevInput, frameMasks, C, Hi, Wi, geom, threshold, fm.update, fm.edt, stream);
    if (st != CB_OK) return st;
    return cbinfer_conv_changed_geom(fm.src, nullptr, 0, nullptr, frameMasks, idx, countDev, prepared, bias, prevOutput, C,
                                     Hi, Wi, K, geom, relu, workspace, dtype, stream);
}

}  // extern "C"
