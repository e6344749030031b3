// WaveMLP's phase-aware token mixing (PATM, wave_mlp.py:46-60) after its 1 x 1 convolutions: ReLU(theta), the cos / sin phase modulation of
// x_h / x_w and the two grouped 7-tap convolutions tfc_h (1 x 7, along W) and tfc_w (7 x 1, along H) in one pass (mlpk.h mlpk_wave_patm).
//
// Pairing (groups = C over the 2C concatenated channels [x cos(theta) | x sin(theta)]): output channel g reads concatenated channels 2g and
// 2g + 1, so for g < C/2 it is the cos of source channels 2g, 2g + 1 and for g >= C/2 the sin of source channels 2g - C, 2g - C + 1.
// A lane owns four source channels s = 4q .. 4q + 3 of one line (a row of the map for the h branch, a column for the w branch): their
// cos products feed outputs 2q, 2q + 1 and their sin products outputs C/2 + 2q, C/2 + 2q + 1 -- the lane's 56 tap weights stay in registers.
// The lane walks its line once: at position p it loads theta and x (one 4-element vector each), forms the eight products in fp32 (OCML
// sincosf, full range reduction) and adds them into the seven outputs p - 3 .. p + 3 they reach, held in a window of seven accumulators that
// moves by one position per step; output p - 3 is then complete and stored (one rounding).  Every product is formed exactly once, and no halo is re-read.
// Workgroups [0, blocks_h) carry h-branch lines, the rest w-branch lines, so a wave's lines all have the same length.
#include "mlpk_common.h"

namespace mlpk {

template <typename T> struct wv4 { typedef T __attribute__((ext_vector_type(4))) type; };
template <typename T> struct wv2 { typedef T __attribute__((ext_vector_type(2))) type; };

template <typename T>
__global__ void __launch_bounds__(256) wave_patm_kernel(const T* __restrict__ y, int64_t ldy, const float* __restrict__ wh,
                                                        const float* __restrict__ ww, T* __restrict__ oh, T* __restrict__ ow, int64_t ldo,
                                                        int H, int W, int C, int64_t lanes_h, int64_t blocks_h, int64_t lanes_w) {
    typedef typename wv4<T>::type v4;
    typedef typename wv2<T>::type v2;
    const bool hb = (int64_t)blockIdx.x < blocks_h;
    const int64_t id = hb ? (int64_t)blockIdx.x * 256 + threadIdx.x : ((int64_t)blockIdx.x - blocks_h) * 256 + threadIdx.x;
    if (id >= (hb ? lanes_h : lanes_w)) return;
    const int nq = C >> 2;
    const int q = (int)(id % nq);
    const int64_t line = id / nq;
    int L;
    int64_t row0, step;
    const float* wt;
    T* out;
    int col_t, col_x;
    if (hb) {                                   // line = b * H + y, walking x
        L = W, row0 = line * W, step = 1, wt = wh, out = oh, col_t = 0, col_x = 2 * C;
    } else {                                    // line = b * W + x, walking y
        const int64_t b = line / W;
        const int x = (int)(line - b * W);
        L = H, row0 = b * H * W + x, step = W, wt = ww, out = ow, col_t = C, col_x = 3 * C;
    }
    // weights (C, 2, 7): [output][concatenated input 2g + i][tap]; this lane's four outputs: cos 2q, 2q + 1; sin C/2 + 2q, C/2 + 2q + 1
    float wk[4][2][7];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int g = (o < 2 ? 0 : C / 2) + 2 * q + (o & 1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 7; ++k) wk[o][i][k] = wt[g * 14 + i * 7 + k];
    }
    float acc[7][4];                            // acc[i]: output p - 3 + i at step p
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[i][o] = 0.f;
    const T* src = y + row0 * ldy + 4 * q;
    const int64_t sstep = step * ldy;
    T* dst = out + row0 * ldo + 2 * q;
    const int64_t dstep = step * ldo;
    const int half = C / 2;
    v4 tn = *reinterpret_cast<const v4*>(src + col_t);
    v4 xn = *reinterpret_cast<const v4*>(src + col_x);
#pragma unroll 1
    for (int p = 0; p < L + 3; ++p) {
        if (p < L) {
            const v4 tc = tn, xc = xn;
            if (p + 1 < L) {                    // the next position's operands in flight while this one is computed
                tn = *reinterpret_cast<const v4*>(src + (int64_t)(p + 1) * sstep + col_t);
                xn = *reinterpret_cast<const v4*>(src + (int64_t)(p + 1) * sstep + col_x);
            }
            float pc[4], ps[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float th = __builtin_fmaxf(to_f32<T>(tc[e]), 0.f);
                float sn, cs;
                sincosf(th, &sn, &cs);
                const float xv = to_f32<T>(xc[e]);
                pc[e] = xv * cs;
                ps[e] = xv * sn;
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) {       // the product at p reaches output p + 3 - k through tap k
                float* a = acc[6 - k];
                a[0] += wk[0][0][k] * pc[0] + wk[0][1][k] * pc[1];
                a[1] += wk[1][0][k] * pc[2] + wk[1][1][k] * pc[3];
                a[2] += wk[2][0][k] * ps[0] + wk[2][1][k] * ps[1];
                a[3] += wk[3][0][k] * ps[2] + wk[3][1][k] * ps[3];
            }
        }
        if (p >= 3) {                           // output p - 3 is complete: every product that reaches it has been added
            T* d = dst + (int64_t)(p - 3) * dstep;
            *reinterpret_cast<v2*>(d) = v2{from_f32<T>(acc[0][0]), from_f32<T>(acc[0][1])};
            *reinterpret_cast<v2*>(d + half) = v2{from_f32<T>(acc[0][2]), from_f32<T>(acc[0][3])};
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[i][o] = acc[i + 1][o];
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[6][o] = 0.f;
    }
}

}  // namespace mlpk

extern "C" int mlpk_wave_patm_supported(int dtype, int B, int H, int W, int C) {
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return 0;
    return B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0;
}

extern "C" int mlpk_wave_patm(int dtype, const void* y, int64_t ldy, const float* wh, const float* ww, void* out_h, void* out_w, int64_t ldo,
                              int B, int H, int W, int C, void* stream) {
    using namespace mlpk;
    if (!y || !wh || !ww || !out_h || !out_w) return MLPK_ENULL;
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (!mlpk_wave_patm_supported(dtype, B, H, W, C) || ldy < 5 * (int64_t)C || ldo < C) return MLPK_ESHAPE;
    const int esz = dtype == MLPK_F32 ? 4 : 2;
    if (((uintptr_t)y % (4 * esz)) || ldy % 4 || ((uintptr_t)out_h % (2 * esz)) || ((uintptr_t)out_w % (2 * esz)) || ldo % 2 ||
        ((uintptr_t)wh % 4) || ((uintptr_t)ww % 4))
        return MLPK_EALIGN;
    const int64_t nq = C / 4;
    const int64_t lanes_h = (int64_t)B * H * nq, lanes_w = (int64_t)B * W * nq;
    const int64_t blocks_h = (lanes_h + 255) / 256, blocks = blocks_h + (lanes_w + 255) / 256;
    if (blocks > 0x7fffffff) return MLPK_ESHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define WP(TT) hipLaunchKernelGGL((wave_patm_kernel<TT>), dim3((unsigned)blocks), dim3(256), 0, s, (const TT*)y, ldy, wh, ww, (TT*)out_h, (TT*)out_w, \
                                  ldo, H, W, C, lanes_h, blocks_h, lanes_w)
    switch (dtype) {
        case MLPK_F32: WP(float); break;
        case MLPK_F16: WP(f16_t); break;
        default: WP(bf16_t); break;
    }
#undef WP
    MLPK_LAUNCH_CHECK();
    return 0;
}
