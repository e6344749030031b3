// Sequencer2D's BiLSTM2D recurrence (sequencer.py:31-46), one bidirectional LSTM along one axis of a channel-last map per launch (mlpk.h
// mlpk_lstm_scan).  The input projections W_ih x + b_ih + b_hh of both directions are an ordinary GEMM's output; what is left is the chain of
// L dependent steps  z = xp + W_hh h_{t-1},  c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g),  h_t = sigmoid(o) tanh(c_t).
//   A workgroup owns 16 MT sequences of ONE direction (blockIdx.y) for all L steps; it has hid / 16 waves, and wave w owns hidden units
//   [16 w, 16 w + 16) of every sequence: its rows of W_hh -- four gates x 16 units x hid -- are loaded ONCE and stay in registers as the A
//   fragments of the matrix instruction (hid = 96, 16-bit: 48 VGPRs; fp32: 96).  Nothing of W_hh lies in LDS.
//   Per step   D[unit][sequence] = W_hh[gate rows of the unit tile][k] h[sequence][k], one 16 x 16 tile per gate, fp32 accumulation that starts
//   from xp: v_mfma_f32_16x16x16 (f16 / bf16, K = 16: hid = 48 is three whole steps, no padding) or v_mfma_f32_16x16x4_f32 (fp32, a true
//   fp32 product).  Lane l receives D[4 (l >> 4) + i][l & 15], i = 0 .. 3, of each gate: all four gates of FOUR CONSECUTIVE hidden units of one
//   sequence.  So xp is read, and h written (to memory and to LDS), as one 8-byte (16-bit) or 16-byte (fp32) vector per gate, c stays in four
//   fp32 registers per 16-sequence tile for the whole sequence, and the gate math needs no exchange between lanes.
//   h is double-buffered in LDS as [sequence][hid + 4] in the storage type: a step reads buffer t & 1 (the B fragments), writes its rounded h_t to
//   the other one, and ONE barrier ends the step.  xp of step t + 1 is requested before step t's products.
//   The reverse direction walks l = L - 1 .. 0 with its own weights and xp columns and writes at its own l: the same instructions.
// A tail workgroup's missing sequences repeat the last real one (every address is inside the map) and store nothing.  Columns of the product are
// sequences, so no sequence sees another one: a NaN stays where it is.
#include "mlpk_common.h"

#include <math.h>

namespace mlpk {

struct LstmArgs {
    const void* xp;
    const void* whh;
    void* out;
    int64_t ldx, ldo, nseq;           // row pitches in elements; sequences per direction (B Q)
    int xoff, ooff, H, W, L, Q, axis;
};

template <typename T> using vec4_t = T __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

// a lane's operand fragment of one matrix instruction: EPL consecutive k
template <typename T> struct lstm_frag { typedef vec4_t<T> type; static constexpr int EPL = 4; };
template <> struct lstm_frag<float> { typedef float type; static constexpr int EPL = 1; };

__device__ __forceinline__ f32x4 lstm_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 lstm_mfma(vec4_t<f16_t> a, vec4_t<f16_t> b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 lstm_mfma(vec4_t<bf16_t> a, vec4_t<bf16_t> b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}

// sigmoid and tanh: every finite x gives a finite result -- an exp that overflows ends in 1 / inf = 0, one that underflows in 1 / 1.
// fp32 storage: evaluated in fp64 and rounded once, so a gate carries half an ulp instead of the two to four ulps of a chain of fp32 libm calls
// (tests/test_gpu_sequencer.py holds fp32 results to four times the distance of torch's own fp32 LSTM from fp64, a handful of ulps in all);
// the products and the cell state stay fp32.  16-bit storage: the hardware exp2 and reciprocal (1 ulp each, far below half an ulp of the
// rounded h).
template <bool PRECISE> __device__ __forceinline__ float lstm_sigmoid(float x) {
    if constexpr (PRECISE) return (float)(1.0 / (1.0 + exp(-(double)x)));
    else return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
template <bool PRECISE> __device__ __forceinline__ float lstm_tanh(float x) {
    if constexpr (PRECISE) return (float)tanh((double)x);
    else return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)), 1.0f);
}

template <typename T, int HID, int MT>
__global__ void __launch_bounds__(HID * 4) lstm_scan_kernel(const LstmArgs p) {
    typedef typename lstm_frag<T>::type frag_t;
    constexpr int EPL = lstm_frag<T>::EPL, KS = 4 * EPL, NK = HID / KS;
    constexpr int LDH = HID + 4;                                      // (rows stay whole 8- / 16-byte vectors)
    constexpr bool PRECISE = sizeof(T) == 4;
    __shared__ __attribute__((aligned(16))) T hs[2][MT * 16][LDH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kq = lane >> 4;
    const int d = blockIdx.y;                                         // 0 forward, 1 reverse
    const int u = wave * 16 + 4 * kq;                                 // this lane's hidden units u .. u + 3
    const T* __restrict__ xp = reinterpret_cast<const T*>(p.xp);
    T* __restrict__ out = reinterpret_cast<T*>(p.out);

    // W_hh of this direction, row-major (4 hid, hid): the A fragments of this wave's unit tile, all gates, all K steps
    const T* __restrict__ w = reinterpret_cast<const T*>(p.whh) + (size_t)d * 4 * HID * HID;
    frag_t a[4][NK];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) a[g][ks] = *reinterpret_cast<const frag_t*>(w + (size_t)(g * HID + wave * 16 + n) * HID + ks * KS + kq * EPL);

    // this lane's sequence of each 16-sequence tile: its first pixel and the pixel step along the line
    int64_t base[MT];
    bool live[MT];
    const int64_t step = p.axis == 0 ? p.W : 1;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int64_t s = (int64_t)blockIdx.x * (16 * MT) + m * 16 + n;
        live[m] = s < p.nseq;
        const int64_t sc = live[m] ? s : p.nseq - 1;
        const int64_t b = sc / p.Q, q = sc - b * p.Q;
        base[m] = p.axis == 0 ? b * p.H * p.W + q : (b * p.H + q) * p.W;
    }
    const int xcol = p.xoff + d * 4 * HID + u, ocol = p.ooff + d * HID + u;
    auto load_x = [&](int t, vec4_t<T> (&x)[MT][4]) {
        const int l = d ? p.L - 1 - t : t;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) x[m][g] = *reinterpret_cast<const vec4_t<T>*>(xp + (base[m] + l * step) * p.ldx + xcol + g * HID);
    };

    for (int i = tid; i < MT * 16 * LDH; i += HID * 4) (&hs[0][0][0])[i] = from_f32<T>(0.0f);         // h_{-1} = 0
    float c[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) c[m][i] = 0.0f;
    vec4_t<T> x[MT][4], xn[MT][4];
    load_x(0, x);
    __syncthreads();

    for (int t = 0; t < p.L; ++t) {
        const int cur = t & 1;
        load_x(t + 1 < p.L ? t + 1 : t, xn);                          // (the last step requests its own again: no branch around the loads)
        f32x4 acc[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[m][g] = f32x4{to_f32(x[m][g][0]), to_f32(x[m][g][1]), to_f32(x[m][g][2]), to_f32(x[m][g][3])};
#pragma unroll
        for (int ks = 0; ks < NK; ++ks)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const frag_t b = *reinterpret_cast<const frag_t*>(&hs[cur][m * 16 + n][ks * KS + kq * EPL]);
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[m][g] = lstm_mfma(a[g][ks], b, acc[m][g]);
            }
        const int l = d ? p.L - 1 - t : t;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            vec4_t<T> h;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ig = lstm_sigmoid<PRECISE>(acc[m][0][i]), fg = lstm_sigmoid<PRECISE>(acc[m][1][i]);
                const float gg = lstm_tanh<PRECISE>(acc[m][2][i]), og = lstm_sigmoid<PRECISE>(acc[m][3][i]);
                c[m][i] = __builtin_fmaf(fg, c[m][i], ig * gg);         // (spelled out: under -ffp-contract=fast the unrolled copies of a*b + c*d need not contract alike)
                h[i] = from_f32<T>(og * lstm_tanh<PRECISE>(c[m][i]));  // rounded ONCE: what is stored is the next step's operand
            }
            *reinterpret_cast<vec4_t<T>*>(&hs[cur ^ 1][m * 16 + n][u]) = h;
            if (live[m]) *reinterpret_cast<vec4_t<T>*>(out + (base[m] + l * step) * p.ldo + ocol) = h;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) x[m][g] = xn[m][g];
    }
}

template <typename T, int HID>
static int lstm_launch_hid(const LstmArgs& a, void* stream) {
    constexpr int MT = sizeof(T) == 2 ? 2 : 1;                        // 16-sequence tiles per workgroup (fp32: W_hh alone is 96 VGPRs at hid = 96)
    const int64_t groups = (a.nseq + 16 * MT - 1) / (16 * MT);
    if (groups > 0x7fffffffLL) return MLPK_ESHAPE;
    hipLaunchKernelGGL((lstm_scan_kernel<T, HID, MT>), dim3((unsigned)groups, 2), dim3(HID * 4), 0, reinterpret_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

template <typename T>
static int lstm_launch(const LstmArgs& a, int hid, void* stream) {
    switch (hid) {
        case 16: return lstm_launch_hid<T, 16>(a, stream);
        case 32: return lstm_launch_hid<T, 32>(a, stream);
        case 48: return lstm_launch_hid<T, 48>(a, stream);
        default: return lstm_launch_hid<T, 96>(a, stream);
    }
}

}  // namespace mlpk

using namespace mlpk;

extern "C" int mlpk_lstm_scan_supported(int dtype, int L, int hid) {
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return 0;
    return L >= 1 && (hid == 16 || hid == 32 || hid == 48 || hid == 96);
}

extern "C" int mlpk_lstm_scan(int dtype, const void* xp, int64_t xp_pitch, int xp_off, const void* whh, void* out, int64_t out_pitch, int out_off,
                              int B, int H, int W, int hid, int axis, void* stream) {
    if (!xp || !whh || !out) return MLPK_ENULL;
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (B <= 0 || H <= 0 || W <= 0 || (axis != 0 && axis != 1)) return MLPK_ESHAPE;
    if (!mlpk_lstm_scan_supported(dtype, axis ? W : H, hid)) return MLPK_ESHAPE;
    if (xp_off < 0 || out_off < 0 || xp_pitch < (int64_t)xp_off + 8 * hid || out_pitch < (int64_t)out_off + 2 * hid) return MLPK_ESHAPE;
    const int64_t es = dtype == MLPK_F32 ? 4 : 2;
    if (((uintptr_t)xp & 15) || ((uintptr_t)out & 15) || ((uintptr_t)whh & 15) || xp_pitch % 4 || out_pitch % 4 || xp_off % 4 || out_off % 4)
        return MLPK_EALIGN;
    const int64_t rows = (int64_t)B * H * W;
    const uintptr_t x0 = (uintptr_t)xp + (uintptr_t)(xp_off * es), x1 = (uintptr_t)xp + (uintptr_t)(((rows - 1) * xp_pitch + xp_off + 8 * hid) * es);
    const uintptr_t o0 = (uintptr_t)out + (uintptr_t)(out_off * es), o1 = (uintptr_t)out + (uintptr_t)(((rows - 1) * out_pitch + out_off + 2 * hid) * es);
    if (x0 < o1 && o0 < x1) return MLPK_EALIGN;                       // the spans of what is read and what is written overlap
    LstmArgs a;
    a.xp = xp; a.whh = whh; a.out = out;
    a.ldx = xp_pitch; a.ldo = out_pitch;
    a.xoff = xp_off; a.ooff = out_off; a.H = H; a.W = W; a.axis = axis;
    a.L = axis ? W : H; a.Q = axis ? H : W;
    a.nseq = (int64_t)B * a.Q;
    switch (dtype) {
        case MLPK_F32: return lstm_launch<float>(a, hid, stream);
        case MLPK_F16: return lstm_launch<f16_t>(a, hid, stream);
        default: return lstm_launch<bf16_t>(a, hid, stream);
    }
}
