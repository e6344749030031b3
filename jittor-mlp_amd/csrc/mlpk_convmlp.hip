// ConvMLP's three passes over large activations (conv_mlp.py:51-87, 123-126, 166-170; mlpk.h mlpk_ln_dwconv3_nhwc, mlpk_relu_add,
// mlpk_relu_maxpool3s2_nhwc).  All operands are dense channel-last tensors (row pitch = C) moved in 16-byte vectors of EPV channels.
//
//   ln_dwconv3   connect(connect_norm(x)): a workgroup owns LN_TH x LN_TW output pixels of one image and up to LN_VL channel vectors.  It stages
//                the (th + 2) x (tw + 2) halo of its tile in LDS, normalising every pixel ONCE on the way ((x - mean) rstd gamma + beta in fp32,
//                rounded to the storage type: mlpk_norm_apply's expression; pixels outside the map are staged as zeros, which is the padding
//                AFTER the norm), then every thread runs the nine taps of its outputs from LDS.  A thread keeps one channel vector for the
//                whole kernel (vector = tid mod vl, vl a power of two), so its 9 x EPV weights and its gamma / beta live in registers.
//                Tiles at the map's edge are cut to the map: item loops run over the pixels that exist, a 7 x 7 map costs 81 staged pixels.
//   relu_add     out = res + max(y, 0): a grid-stride loop over vectors; each vector is read before it is written, so out may be y or res.
//   relu_maxpool one output vector per thread, the in-map pixels of its 3 x 3 window read through the cache (each input is read 2.25 times, by
//                neighbouring lanes), the maximum started at 0: ReLU and the padding in one.
#include "mlpk_common.h"

namespace mlpk {

constexpr int LN_TH = 8, LN_TW = 16, LN_VL = 8;
constexpr int RELU_GRID_MAX = 2048;               // workgroups of mlpk_relu_add: beyond RELU_GRID_MAX * 256 vectors a thread loops

struct LnDwArgs {
    const void* x;
    void* out;
    const float* mean;   // per pixel, or NULL: 0 / 1
    const float* rstd;
    const float* gamma;  // per channel, or NULL: 1
    const float* beta;   // or NULL: 0
    const float* w;      // [9][C]
    int B, H, W, C;
    int ty, tx, nch;     // tiles along y and x, channel chunks of vl vectors
    int vl, vshift;      // vectors per chunk (1, 2, 4, 8) and its log2
};

// an fp32 value on its own before it is rounded to the storage type (mlpk_raft.hip raft_f32: the identity lane permutation keeps the
// compiler from fusing the multiply-add with the conversion, which would round once where mlpk_norm_apply rounds twice)
__device__ __forceinline__ float cm_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xE4, 0xF, 0xF, false));
}

template <typename T>
__global__ void __launch_bounds__(256) ln_dwconv3_kernel(const LnDwArgs p) {
    constexpr int EPV = 16 / (int)sizeof(T);
    __shared__ u32x4 tile[(LN_TH + 2) * (LN_TW + 2) * LN_VL];
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    T* __restrict__ out = reinterpret_cast<T*>(p.out);
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int ch = bid % p.nch; bid /= p.nch;
    const int txi = bid % p.tx; bid /= p.tx;
    const int tyi = bid % p.ty;
    const int b = bid / p.ty;
    const int y0 = tyi * LN_TH, x0 = txi * LN_TW;
    const int th = min(LN_TH, p.H - y0), tw = min(LN_TW, p.W - x0);
    const int hw = tw + 2;                                            // pixels per staged row
    const int v = tid & (p.vl - 1), slot = tid >> p.vshift, nslots = 256 >> p.vshift;
    const int cv = p.C / EPV;
    const int vg = ch * p.vl + v;                                     // this thread's channel vector
    const bool live = vg < cv;                                        // (the last chunk of a ragged C has idle lanes)
    const int c0 = vg * EPV;
    const int64_t img = (int64_t)b * p.H * p.W;

    // ---- stage: every pixel of the halo normalised once
    if (live) {
        float g[EPV], bt[EPV];
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            g[k] = p.gamma ? p.gamma[c0 + k] : 1.0f;
            bt[k] = p.beta ? p.beta[c0 + k] : 0.0f;
        }
        const int npx = (th + 2) * hw;
        for (int pi = slot; pi < npx; pi += nslots) {
            const int r = pi / hw, q = pi - r * hw;
            const int gy = y0 - 1 + r, gx = x0 - 1 + q;
            T e[EPV];
            if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
                const int64_t pix = img + (int64_t)gy * p.W + gx;
                const u32x4 raw = *reinterpret_cast<const u32x4*>(x + pix * p.C + c0);
                float mu = 0.f, rs = 1.f;
                if (p.mean) { mu = p.mean[pix]; rs = p.rstd[pix]; }
                T t[EPV];
                __builtin_memcpy(t, &raw, 16);
#pragma unroll
                for (int k = 0; k < EPV; ++k) e[k] = from_f32<T>(cm_f32(__builtin_fmaf((to_f32(t[k]) - mu) * rs, g[k], bt[k])));
            } else {
#pragma unroll
                for (int k = 0; k < EPV; ++k) e[k] = from_f32<T>(0.f);    // the padding follows the norm: exactly 0, not beta
            }
            u32x4 pk;
            __builtin_memcpy(&pk, e, 16);
            tile[pi * p.vl + v] = pk;
        }
    }
    __syncthreads();
    if (!live) return;

    // ---- nine taps per output from LDS, fp32, in tap order
    float wt[9][EPV];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < EPV; ++k) wt[t][k] = p.w[(int64_t)t * p.C + c0 + k];
    const int nout = th * tw;
    for (int po = slot; po < nout; po += nslots) {
        const int oy = po / tw, ox = po - oy * tw;
        float acc[EPV];
#pragma unroll
        for (int k = 0; k < EPV; ++k) acc[k] = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const u32x4 raw = tile[((oy + i) * hw + ox + j) * p.vl + v];
                T t[EPV];
                __builtin_memcpy(t, &raw, 16);
#pragma unroll
                for (int k = 0; k < EPV; ++k) acc[k] = __builtin_fmaf(wt[3 * i + j][k], to_f32(t[k]), acc[k]);
            }
        T e[EPV];
#pragma unroll
        for (int k = 0; k < EPV; ++k) e[k] = from_f32<T>(cm_f32(acc[k]));
        const int64_t pix = img + (int64_t)(y0 + oy) * p.W + x0 + ox;
        u32x4 pk;
        __builtin_memcpy(&pk, e, 16);
        *reinterpret_cast<u32x4*>(out + pix * p.C + c0) = pk;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) relu_add_kernel(const T* y, const T* res, T* out, int64_t nvec) {
    constexpr int EPV = 16 / (int)sizeof(T);
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += step) {
        const u32x4 ry = *reinterpret_cast<const u32x4*>(y + i * EPV);
        T a[EPV], r[EPV], e[EPV];
        __builtin_memcpy(a, &ry, 16);
        if (res) {
            const u32x4 rr = *reinterpret_cast<const u32x4*>(res + i * EPV);
            __builtin_memcpy(r, &rr, 16);
        }
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            const float f = to_f32(a[k]);
            const float z = f < 0.f ? 0.f : f;                        // (a NaN stays a NaN, as in torch)
            e[k] = res ? from_f32<T>(to_f32(r[k]) + z) : from_f32<T>(z);
        }
        u32x4 pk;
        __builtin_memcpy(&pk, e, 16);
        *reinterpret_cast<u32x4*>(out + i * EPV) = pk;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) relu_maxpool3s2_kernel(const T* __restrict__ y, T* __restrict__ out, int H, int W, int C, int Ho, int Wo,
                                                              int64_t total) {
    constexpr int EPV = 16 / (int)sizeof(T);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int cv = C / EPV;
    const int vg = (int)(i % cv);
    int64_t rest = i / cv;
    const int xo = (int)(rest % Wo); rest /= Wo;
    const int yo = (int)(rest % Ho);
    const int64_t b = rest / Ho;
    float m[EPV];
#pragma unroll
    for (int k = 0; k < EPV; ++k) m[k] = 0.f;
#pragma unroll
    for (int di = 0; di < 3; ++di) {
        const int gy = 2 * yo - 1 + di;
        if (gy < 0 || gy >= H) continue;
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
            const int gx = 2 * xo - 1 + dj;
            if (gx < 0 || gx >= W) continue;
            const u32x4 raw = *reinterpret_cast<const u32x4*>(y + ((b * H + gy) * W + gx) * C + (int64_t)vg * EPV);
            T t[EPV];
            __builtin_memcpy(t, &raw, 16);
#pragma unroll
            for (int k = 0; k < EPV; ++k) {
                const float f = to_f32(t[k]);
                m[k] = (f > m[k] || f != f) ? f : m[k];               // (a NaN is taken and then kept: torch's max_pool2d propagates it)
            }
        }
    }
    T e[EPV];
#pragma unroll
    for (int k = 0; k < EPV; ++k) e[k] = from_f32<T>(m[k]);
    u32x4 pk;
    __builtin_memcpy(&pk, e, 16);
    *reinterpret_cast<u32x4*>(out + ((b * Ho + yo) * Wo + xo) * C + (int64_t)vg * EPV) = pk;
}

static int cm_dtype(int dtype) { return (dtype == MLPK_F32 || dtype == MLPK_F16 || dtype == MLPK_BF16) ? 0 : MLPK_EDTYPE; }

// the launch plan of mlpk_ln_dwconv3_nhwc: from dtype, H, W and C alone (B only multiplies the grid)
static int ln_dw_plan(int dtype, int B, int H, int W, int C, LnDwArgs* a) {
    if (const int rc = cm_dtype(dtype)) return rc;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return MLPK_ESHAPE;
    const int epv = dtype == MLPK_F32 ? 4 : 8;
    if (C % epv) return MLPK_ESHAPE;
    const int cv = C / epv;
    a->vl = 1; a->vshift = 0;
    while (a->vl < LN_VL && a->vl < cv) { a->vl <<= 1; ++a->vshift; }
    a->B = B; a->H = H; a->W = W; a->C = C;
    a->ty = (H + LN_TH - 1) / LN_TH;
    a->tx = (W + LN_TW - 1) / LN_TW;
    a->nch = (cv + a->vl - 1) / a->vl;
    if ((long long)B * a->ty * a->tx * a->nch > 0x7fffffffLL) return MLPK_ESHAPE;
    return 0;
}

static int pool_plan(int dtype, int B, int H, int W, int C, long long* total) {
    if (const int rc = cm_dtype(dtype)) return rc;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return MLPK_ESHAPE;
    const int epv = dtype == MLPK_F32 ? 4 : 8;
    if (C % epv) return MLPK_ESHAPE;
    const long long Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    *total = (long long)B * Ho * Wo * (C / epv);
    if ((*total + 255) / 256 > 0x7fffffffLL) return MLPK_ESHAPE;
    return 0;
}

}  // namespace mlpk

using namespace mlpk;

extern "C" int mlpk_ln_dwconv3_nhwc_supported(int dtype, int B, int H, int W, int C) {
    LnDwArgs a;
    return ln_dw_plan(dtype, B, H, W, C, &a) == 0;
}

extern "C" int mlpk_ln_dwconv3_nhwc(int dtype, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    const float* w, void* out, int B, int H, int W, int C, void* stream) {
    if (!x || !out || !w || (mean != nullptr) != (rstd != nullptr)) return MLPK_ENULL;
    LnDwArgs a;
    if (const int rc = ln_dw_plan(dtype, B, H, W, C, &a)) return rc;
    if (x == out) return MLPK_ESHAPE;                    // a stencil cannot run in place
    if (((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return MLPK_EALIGN;
    a.x = x; a.out = out; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.w = w;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((long long)B * a.ty * a.tx * a.nch));
    switch (dtype) {
        case MLPK_F32: hipLaunchKernelGGL(ln_dwconv3_kernel<float>, grid, dim3(256), 0, s, a); break;
        case MLPK_F16: hipLaunchKernelGGL(ln_dwconv3_kernel<f16_t>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(ln_dwconv3_kernel<bf16_t>, grid, dim3(256), 0, s, a); break;
    }
    MLPK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mlpk_relu_add_supported(int dtype, int64_t n) {
    if (cm_dtype(dtype)) return 0;
    return n > 0 && n % (dtype == MLPK_F32 ? 4 : 8) == 0;
}

extern "C" int mlpk_relu_add(int dtype, const void* y, const void* res, void* out, int64_t n, void* stream) {
    if (!y || !out) return MLPK_ENULL;
    if (const int rc = cm_dtype(dtype)) return rc;
    const int epv = dtype == MLPK_F32 ? 4 : 8;
    if (n <= 0 || n % epv) return MLPK_ESHAPE;
    if (((uintptr_t)y & 15) || ((uintptr_t)res & 15) || ((uintptr_t)out & 15)) return MLPK_EALIGN;
    const int64_t nvec = n / epv;
    const int64_t want = (nvec + 255) / 256;
    const dim3 grid((unsigned)(want < RELU_GRID_MAX ? want : RELU_GRID_MAX));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (dtype) {
        case MLPK_F32: hipLaunchKernelGGL(relu_add_kernel<float>, grid, dim3(256), 0, s, (const float*)y, (const float*)res, (float*)out, nvec); break;
        case MLPK_F16: hipLaunchKernelGGL(relu_add_kernel<f16_t>, grid, dim3(256), 0, s, (const f16_t*)y, (const f16_t*)res, (f16_t*)out, nvec); break;
        default: hipLaunchKernelGGL(relu_add_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)y, (const bf16_t*)res, (bf16_t*)out, nvec); break;
    }
    MLPK_LAUNCH_CHECK();
    return 0;
}

extern "C" int mlpk_relu_maxpool3s2_nhwc_supported(int dtype, int B, int H, int W, int C) {
    long long total;
    return pool_plan(dtype, B, H, W, C, &total) == 0;
}

extern "C" int mlpk_relu_maxpool3s2_nhwc(int dtype, const void* y, void* out, int B, int H, int W, int C, void* stream) {
    if (!y || !out) return MLPK_ENULL;
    long long total;
    if (const int rc = pool_plan(dtype, B, H, W, C, &total)) return rc;
    if (y == out) return MLPK_ESHAPE;                    // a window cannot run in place
    if (((uintptr_t)y & 15) || ((uintptr_t)out & 15)) return MLPK_EALIGN;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (dtype) {
        case MLPK_F32: hipLaunchKernelGGL(relu_maxpool3s2_kernel<float>, grid, dim3(256), 0, s, (const float*)y, (float*)out, H, W, C, Ho, Wo, (int64_t)total); break;
        case MLPK_F16: hipLaunchKernelGGL(relu_maxpool3s2_kernel<f16_t>, grid, dim3(256), 0, s, (const f16_t*)y, (f16_t*)out, H, W, C, Ho, Wo, (int64_t)total); break;
        default: hipLaunchKernelGGL(relu_maxpool3s2_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)y, (bf16_t*)out, H, W, C, Ho, Wo, (int64_t)total); break;
    }
    MLPK_LAUNCH_CHECK();
    return 0;
}
