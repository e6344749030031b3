// RaftMLP's raft token mixing (raft_mlp.py:114-146, 333-362), the data movement around its two-layer MLP (mlpk.h mlpk_raft_gather_ln /
// mlpk_raft_scatter_add).  The MLP runs over vectors z[j * L + l] that interleave the r = raft_size channel groups j of one channel co
// (channel c = j * Co + co) with one spatial axis l; activations live as channel-last rows x[(b, h, w), c].  For one (b, q) -- q the position on
// the OTHER spatial axis -- the L pixels x C channels of x and the Co rows x (r L) columns of the operand are the same L C numbers, re-laid as r
// transposes of L x Co.  A workgroup owns QT adjacent q of one image and turns them over in LDS:
//   gather   16-byte loads along c (a lane group of 32 = 32 / EPV channel vectors x EPV pixel units), the block's LayerNorm on the way
//            ((x - mean) rstd gamma + beta in fp32, one rounding: mlpk_norm_apply's expression), written TRANSPOSED as dwords tile[c][l unit]
//            -- a 16-bit lane carries two adjacent pixels, so the transposing write is one ds_write_b32 per channel, and with an ODD dword
//            pitch per channel the 32 lanes of a group fall on 32 different banks: bank = (EPV v pitch + unit) mod 32 --; then rows of the
//            operand leave as 16-byte stores, consecutive lanes = consecutive vectors of one row (rows of one q are adjacent in memory).
//   scatter  the reverse: rows of y enter along their columns, the tile is read with the gather's conflict-free dword pattern, and
//            x <- round(float(x) + float(y)) leaves as 16-byte stores along c.
// Both are HBM-bound element moves: one read and one write of the activation (the scatter reads x as well).
#include "mlpk_common.h"

namespace mlpk {

struct RaftArgs {
    void* x;             // (B, H, W, C) channel-last rows at pitch ldx: read by the gather, updated in place by the scatter
    void* a;             // gather: the operand written; scatter: y, the MLP's output read
    int64_t ldx, lda;
    const float* mean;   // per pixel, or NULL: 0 / 1
    const float* rstd;
    const float* gamma;  // per channel (indexed by the activation's channel), or NULL: 1
    const float* beta;   // or NULL: 0
    int kp;              // gather: columns [D, kp) of every row are written as zeros
    int B, H, W, C, r, axis;
    int L, Q, Co, D;     // axis 0: L = H, Q = W; axis 1: L = W, Q = H; Co = C / r; D = r L
    int sl, sq;          // pixel strides of l and q inside an image
    int qt, nqt;         // q per workgroup, workgroups per image
    int lu, p2;          // pixel units per column (two pixels per unit for 16-bit types) and the odd dword pitch of a channel's row in LDS
    int vt, lt;          // lane-group tiles along the channel vectors and along the units
};

constexpr int RAFT_LDS_MAX = 160 * 1024;
constexpr int RAFT_LDS_WANT = 48 * 1024;      // QT is halved until QT columns fit this: three workgroups per CU

// An fp32 result as a value of its own before it is rounded to the storage type, as mlpk_norm_apply and torch round (fp32 first, then the
// storage type).  Left to itself the compiler fuses an fp32 multiply-add and its conversion to f16 into v_fma_mixlo_f16, which rounds once: about
// one element in 2^14 then differs from mlpk_norm_apply's in its last bit.  An identity lane permutation is opaque to that fusion.
__device__ __forceinline__ float raft_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xE4, 0xF, 0xF, false));
}

// the lane-group item i of phase "along c": channel vector v, pixel unit u, column qi of the workgroup (false: an idle lane)
template <int EPV>
__device__ __forceinline__ bool raft_item(const RaftArgs& p, int i, int per_q, int& qi, int& v, int& u) {
    constexpr int VL = 32 / EPV;
    qi = i / per_q;
    const int rem = i - qi * per_q;
    const int tl = rem >> 5, lane = rem & 31;
    const int ltile = tl / p.vt, vtile = tl - ltile * p.vt;
    v = vtile * VL + (lane & (VL - 1));
    u = ltile * EPV + lane / VL;
    return v < p.C / EPV && u < p.lu;
}

template <typename T>
__global__ void __launch_bounds__(256) raft_gather_kernel(const RaftArgs p) {
    constexpr int EPV = 16 / (int)sizeof(T);
    constexpr int PACK = 4 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint32_t* tile = reinterpret_cast<uint32_t*>(smem_raw);           // [qi][c][p2] dwords
    const T* tile_t = reinterpret_cast<const T*>(smem_raw);
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    T* __restrict__ a = reinterpret_cast<T*>(p.a);
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.nqt;
    const int q0 = (blockIdx.x - b * p.nqt) * p.qt;
    const int nq = min(p.qt, p.Q - q0);
    const int64_t img = (int64_t)b * p.H * p.W;
    const int per_q = p.lt * p.vt * 32;
    for (int i = tid; i < nq * per_q; i += 256) {
        int qi, v, u;
        if (!raft_item<EPV>(p, i, per_q, qi, v, u)) continue;
        const int c0 = v * EPV;
        float g[EPV], bt[EPV];
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            g[k] = p.gamma ? p.gamma[c0 + k] : 1.0f;
            bt[k] = p.beta ? p.beta[c0 + k] : 0.0f;
        }
        T e[PACK][EPV];
#pragma unroll
        for (int s = 0; s < PACK; ++s) {
            const int l = u * PACK + s;
            const bool in = l < p.L;
            const int64_t pix = img + (int64_t)(in ? l : 0) * p.sl + (int64_t)(q0 + qi) * p.sq;
            const u32x4 raw = *reinterpret_cast<const u32x4*>(x + pix * p.ldx + c0);
            float mu = 0.f, rs = 1.f;
            if (p.mean) { mu = p.mean[pix]; rs = p.rstd[pix]; }
            T t[EPV];
            __builtin_memcpy(t, &raw, 16);
#pragma unroll
            for (int k = 0; k < EPV; ++k) e[s][k] = in ? from_f32<T>(raft_f32(__builtin_fmaf((to_f32(t[k]) - mu) * rs, g[k], bt[k]))) : from_f32<T>(0.f);   // (norm_apply_tile_kernel's form)
        }
        uint32_t* dst = tile + ((size_t)qi * p.C + c0) * p.p2 + u;
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            T pr[PACK];
#pragma unroll
            for (int s = 0; s < PACK; ++s) pr[s] = e[s][k];
            uint32_t w;
            __builtin_memcpy(&w, pr, 4);
            dst[(size_t)k * p.p2] = w;
        }
    }
    __syncthreads();
    const int nvo = (p.kp + EPV - 1) / EPV;                           // 16-byte pieces of an operand row (the last one may be partial)
    const int total = nq * p.Co * nvo;
    const int rowp = p.p2 * PACK;                                     // a channel's row in LDS, in elements
    for (int i = tid; i < total; i += 256) {
        const int row = i / nvo, dv = i - row * nvo;
        const int qi = row / p.Co, co = row - qi * p.Co;
        const int d0 = dv * EPV;
        int j = d0 / p.L, l = d0 - j * p.L;
        T e[EPV];
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            if (d0 + k < p.D) {
                e[k] = tile_t[((size_t)qi * p.C + (size_t)j * p.Co + co) * rowp + l];
                if (++l == p.L) { l = 0; ++j; }
            } else {
                e[k] = from_f32<T>(0.f);
            }
        }
        T* o = a + (((int64_t)b * p.Q + q0 + qi) * p.Co + co) * p.lda + d0;
        if (d0 + EPV <= p.kp) {
            *reinterpret_cast<u32x4*>(o) = *reinterpret_cast<const u32x4*>(e);
        } else {
            for (int k = 0; d0 + k < p.kp; ++k) o[k] = e[k];
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) raft_scatter_kernel(const RaftArgs p) {
    constexpr int EPV = 16 / (int)sizeof(T);
    constexpr int PACK = 4 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const uint32_t* tile = reinterpret_cast<const uint32_t*>(smem_raw);
    T* tile_t = reinterpret_cast<T*>(smem_raw);
    T* x = reinterpret_cast<T*>(p.x);
    const T* __restrict__ y = reinterpret_cast<const T*>(p.a);
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.nqt;
    const int q0 = (blockIdx.x - b * p.nqt) * p.qt;
    const int nq = min(p.qt, p.Q - q0);
    const int64_t img = (int64_t)b * p.H * p.W;
    const int nvo = (p.D + EPV - 1) / EPV;
    const int total = nq * p.Co * nvo;
    const int rowp = p.p2 * PACK;
    for (int i = tid; i < total; i += 256) {
        const int row = i / nvo, dv = i - row * nvo;
        const int qi = row / p.Co, co = row - qi * p.Co;
        const int d0 = dv * EPV;
        const T* src = y + (((int64_t)b * p.Q + q0 + qi) * p.Co + co) * p.lda + d0;
        T e[EPV];
        if (d0 + EPV <= p.D) {
            *reinterpret_cast<u32x4*>(e) = *reinterpret_cast<const u32x4*>(src);
        } else {                                                      // columns at or beyond D are never read
#pragma unroll
            for (int k = 0; k < EPV; ++k) e[k] = d0 + k < p.D ? src[k] : from_f32<T>(0.f);
        }
        int j = d0 / p.L, l = d0 - j * p.L;
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            if (d0 + k < p.D) {
                tile_t[((size_t)qi * p.C + (size_t)j * p.Co + co) * rowp + l] = e[k];
                if (++l == p.L) { l = 0; ++j; }
            }
        }
    }
    __syncthreads();
    const int per_q = p.lt * p.vt * 32;
    for (int i = tid; i < nq * per_q; i += 256) {
        int qi, v, u;
        if (!raft_item<EPV>(p, i, per_q, qi, v, u)) continue;
        const int c0 = v * EPV;
        const uint32_t* src = tile + ((size_t)qi * p.C + c0) * p.p2 + u;
        T add[PACK][EPV];
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            const uint32_t w = src[(size_t)k * p.p2];
            T pr[PACK];
            __builtin_memcpy(pr, &w, 4);
#pragma unroll
            for (int s = 0; s < PACK; ++s) add[s][k] = pr[s];
        }
#pragma unroll
        for (int s = 0; s < PACK; ++s) {
            const int l = u * PACK + s;
            if (l >= p.L) continue;                                   // (the odd pixel of the last unit: its half of the dword was never written)
            const int64_t pix = img + (int64_t)l * p.sl + (int64_t)(q0 + qi) * p.sq;
            T* px = x + pix * p.ldx + c0;
            T t[EPV];
            *reinterpret_cast<u32x4*>(t) = *reinterpret_cast<const u32x4*>(px);
#pragma unroll
            for (int k = 0; k < EPV; ++k) t[k] = from_f32<T>(raft_f32(to_f32(t[k]) + to_f32(add[s][k])));
            *reinterpret_cast<u32x4*>(px) = *reinterpret_cast<const u32x4*>(t);
        }
    }
}

// shape checks shared by both entries and mlpk_raft_supported; fills the derived fields
static int raft_geometry(int dtype, int B, int H, int W, int C, int r, int axis, RaftArgs* a) {
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || r <= 0 || C % r || (axis != 0 && axis != 1)) return MLPK_ESHAPE;
    const int epv = dtype == MLPK_F32 ? 4 : 8, pack = dtype == MLPK_F32 ? 1 : 2;
    if (C % epv) return MLPK_ESHAPE;
    a->B = B; a->H = H; a->W = W; a->C = C; a->r = r; a->axis = axis;
    a->L = axis == 0 ? H : W;
    a->Q = axis == 0 ? W : H;
    a->sl = axis == 0 ? W : 1;
    a->sq = axis == 0 ? 1 : W;
    a->Co = C / r;
    if ((long long)r * a->L > 0x7fffffffLL / 4) return MLPK_ESHAPE;
    a->D = r * a->L;
    a->lu = (a->L + pack - 1) / pack;
    a->p2 = a->lu | 1;
    const long long col = (long long)C * a->p2 * 4;                   // one (b, q) column in LDS
    if (col > RAFT_LDS_MAX) return MLPK_ESHAPE;
    a->qt = 4;
    while (a->qt > 1 && a->qt * col > RAFT_LDS_WANT) a->qt >>= 1;
    a->nqt = (a->Q + a->qt - 1) / a->qt;
    if ((long long)B * a->nqt > 0x7fffffffLL) return MLPK_ESHAPE;
    a->vt = (C / epv + 32 / epv - 1) / (32 / epv);
    a->lt = (a->lu + epv - 1) / epv;
    return 0;
}

template <typename K>
static int raft_launch(K kernel, const RaftArgs& a, int dtype, void* stream) {
    const int lds = a.qt * a.C * a.p2 * 4;
    return launch_lds(kernel, dim3((unsigned)(a.B * a.nqt)), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
}

}  // namespace mlpk

using namespace mlpk;

extern "C" int mlpk_raft_supported(int dtype, int H, int W, int C, int r, int axis) {
    RaftArgs a;
    return raft_geometry(dtype, 1, H, W, C, r, axis, &a) == 0;
}

extern "C" int mlpk_raft_gather_ln(int dtype, const void* x, int64_t x_pitch, const float* mean, const float* rstd, const float* gamma,
                                   const float* beta, void* a_out, int64_t a_pitch, int kp, int B, int H, int W, int C, int r, int axis,
                                   void* stream) {
    if (!x || !a_out || (mean != nullptr) != (rstd != nullptr)) return MLPK_ENULL;
    RaftArgs a;
    if (const int rc = raft_geometry(dtype, B, H, W, C, r, axis, &a)) return rc;
    if (kp < a.D || kp > a_pitch || x_pitch < C) return MLPK_ESHAPE;
    const int epv = dtype == MLPK_F32 ? 4 : 8;
    if (((uintptr_t)x & 15) || ((uintptr_t)a_out & 15) || x_pitch % epv || a_pitch % epv) return MLPK_EALIGN;
    a.x = const_cast<void*>(x); a.a = a_out; a.ldx = x_pitch; a.lda = a_pitch; a.kp = kp;
    a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
    switch (dtype) {
        case MLPK_F32: return raft_launch(raft_gather_kernel<float>, a, dtype, stream);
        case MLPK_F16: return raft_launch(raft_gather_kernel<f16_t>, a, dtype, stream);
        default: return raft_launch(raft_gather_kernel<bf16_t>, a, dtype, stream);
    }
}

extern "C" int mlpk_raft_scatter_add(int dtype, void* x, int64_t x_pitch, const void* y, int64_t y_pitch, int B, int H, int W, int C, int r,
                                     int axis, void* stream) {
    if (!x || !y) return MLPK_ENULL;
    RaftArgs a;
    if (const int rc = raft_geometry(dtype, B, H, W, C, r, axis, &a)) return rc;
    if (y_pitch < a.D || x_pitch < C) return MLPK_ESHAPE;
    const int epv = dtype == MLPK_F32 ? 4 : 8;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || x_pitch % epv || y_pitch % epv) return MLPK_EALIGN;
    a.x = x; a.a = const_cast<void*>(y); a.ldx = x_pitch; a.lda = y_pitch; a.kp = a.D;
    a.mean = a.rstd = a.gamma = a.beta = nullptr;
    switch (dtype) {
        case MLPK_F32: return raft_launch(raft_scatter_kernel<float>, a, dtype, stream);
        case MLPK_F16: return raft_launch(raft_scatter_kernel<f16_t>, a, dtype, stream);
        default: return raft_launch(raft_scatter_kernel<bf16_t>, a, dtype, stream);
    }
}
