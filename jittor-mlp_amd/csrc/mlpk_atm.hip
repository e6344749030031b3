// ActiveMLP's active token mixer (active_mlp.py:65-127), the sampling in front of its three products (mlpk.h mlpk_atm_sample).  ATMOp hands
// torchvision's deform_conv2d a 1 x 1 kernel and a learned, real-valued offset per pixel and channel along ONE axis: bilinear sampling with the
// other offset identically zero is linear interpolation between two neighbours on a line of the map, zero outside it.  The operand is
// v = LayerNorm(x) rounded to the storage type (mlpk_norm_apply's expression), never stored on its own:
//   a workgroup owns one line of one image -- a row (b, y, .) for the w branch, a column (b, ., x) for the h branch -- and a chunk of channels;
//   phase 1   16-byte loads of x along c, normalised in fp32, rounded, staged in LDS as tile[l][c] (consecutive lanes = consecutive 16-byte
//             pieces: no bank conflict); the row workgroups store the same vectors as out_c;
//   phase 2   per (pixel, 16-byte channel vector): the offset of each channel's group, atm_tap (mlpk_atm_tap.h), the two taps from LDS,
//             w0 v0 + w1 v1 in fp32, one rounding, a 16-byte store.
// x is read twice (rows and columns; a column workgroup's reads are one whole 128-byte line per pixel for 64 16-bit channels), the offsets once,
// every output written once.  An image's map fits L2, so the second read of x is served from there.
#include "mlpk_atm_tap.h"
#include "mlpk_common.h"

namespace mlpk {

struct AtmArgs {
    const void* x;
    const void* off;
    void* out_w;
    void* out_h;
    void* out_c;
    int64_t ldx, ldoff, ldo;
    const float* mean;   // per pixel, or NULL: 0 / 1
    const float* rstd;
    const float* gamma;  // per channel, or NULL: 1
    const float* beta;   // or NULL: 0
    int B, H, W, C, share;
    int cc, nchunk;      // channels per workgroup, workgroups per line
    int nrow;            // row workgroups (B H nchunk, or 0 when neither out_w nor out_c is asked for); the column workgroups follow
};

constexpr int ATM_LDS_MAX = 64 * 1024;

// (mlpk_raft.hip raft_f32: keeps the fp32 result a value of its own, so that fma + conversion are not fused into one rounding and v has
// mlpk_norm_apply's bits)
__device__ __forceinline__ float atm_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xE4, 0xF, 0xF, false));
}

// G adjacent elements of the staged line as ONE LDS read (2 .. 16 bytes; the address is aligned to it)
template <typename T, int G>
__device__ __forceinline__ void atm_lds_read(const T* src, T (&dst)[G]) {
    constexpr int BYTES = G * (int)sizeof(T);
    if constexpr (BYTES == 16) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(src);
        __builtin_memcpy(dst, &w, 16);
    } else if constexpr (BYTES == 8) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(src);
        __builtin_memcpy(dst, &w, 8);
    } else if constexpr (BYTES == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(src);
        __builtin_memcpy(dst, &w, 4);
    } else {
        dst[0] = src[0];
    }
}

// G = the number of adjacent channels of a 16-byte vector that are known to share one offset column: the largest power of two that divides
// `share`, at most the vector's length (vectors start at multiples of their length, and so does the h branch's column base C).  One offset,
// one tap computation and one LDS read per row serve G channels.
template <typename T, int G>
__global__ void __launch_bounds__(256) atm_sample_kernel(const AtmArgs p) {
    constexpr int EPV = 16 / (int)sizeof(T);
    static_assert(G >= 1 && G <= EPV && EPV % G == 0, "G divides the vector");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* tile = reinterpret_cast<T*>(smem_raw);                         // [l][cc]
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ off = reinterpret_cast<const T*>(p.off);
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int axis = bid >= p.nrow ? 1 : 0;                           // 0: a row, the w branch (and out_c); 1: a column, the h branch
    if (axis) bid -= p.nrow;
    const int L = axis ? p.H : p.W, Q = axis ? p.W : p.H;
    const int chunk = bid % p.nchunk;
    const int line = bid / p.nchunk;
    const int b = line / Q, q = line - b * Q;
    const int c_lo = chunk * p.cc;
    const int nv = min(p.cc, p.C - c_lo) / EPV;
    const int64_t base = axis ? (int64_t)b * p.H * p.W + q : ((int64_t)b * p.H + q) * p.W;
    const int64_t step = axis ? p.W : 1;
    T* out_c = axis ? nullptr : reinterpret_cast<T*>(p.out_c);
    T* out_s = reinterpret_cast<T*>(axis ? p.out_h : p.out_w);
    const int items = L * nv;
    for (int i = tid; i < items; i += 256) {
        const int l = i / nv, v = i - l * nv;
        const int c0 = c_lo + v * EPV;
        const int64_t pix = base + (int64_t)l * step;
        const u32x4 raw = *reinterpret_cast<const u32x4*>(x + pix * p.ldx + c0);
        float mu = 0.f, rs = 1.f;
        if (p.mean) { mu = p.mean[pix]; rs = p.rstd[pix]; }
        T t[EPV], e[EPV];
        __builtin_memcpy(t, &raw, 16);
#pragma unroll
        for (int k = 0; k < EPV; ++k) {
            const float g = p.gamma ? p.gamma[c0 + k] : 1.0f;
            const float bt = p.beta ? p.beta[c0 + k] : 0.0f;
            e[k] = from_f32<T>(atm_f32(__builtin_fmaf((to_f32(t[k]) - mu) * rs, g, bt)));   // (norm_apply_tile_kernel's form)
        }
        u32x4 pk;
        __builtin_memcpy(&pk, e, 16);
        *reinterpret_cast<u32x4*>(tile + (size_t)l * p.cc + v * EPV) = pk;
        if (out_c) *reinterpret_cast<u32x4*>(out_c + pix * p.ldo + c0) = pk;
    }
    if (!out_s) return;                                               // (uniform: only out_c was asked of this row)
    __syncthreads();
    const int obase = axis ? p.C : 0;                                 // the h branch's offsets are columns (C + c) / share
    for (int i = tid; i < items; i += 256) {
        const int l = i / nv, v = i - l * nv;
        const int c0 = c_lo + v * EPV;
        const int64_t pix = base + (int64_t)l * step;
        const T* orow = off + pix * p.ldoff;
        const T* col = tile + v * EPV;
        T e[EPV];
#pragma unroll
        for (int k = 0; k < EPV; k += G) {
            const AtmTap tap = atm_tap(to_f32(orow[(obase + c0 + k) / p.share]), l, L);
            const bool add1 = tap.ok1 && tap.w1 != 0.0f;              // (a tap of weight 0 is not added: an integer offset returns v's bits, -0 included)
            T v0[G], v1[G];
            if (tap.ok0) atm_lds_read<T, G>(col + (size_t)tap.i0 * p.cc + k, v0);
            if (add1) atm_lds_read<T, G>(col + (size_t)tap.i1 * p.cc + k, v1);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                float r = 0.0f;
                if (tap.ok0) r = tap.w0 * to_f32(v0[j]);
                if (add1) r = __builtin_fmaf(tap.w1, to_f32(v1[j]), r);
                e[k + j] = from_f32<T>(r);
            }
        }
        u32x4 pk;
        __builtin_memcpy(&pk, e, 16);
        *reinterpret_cast<u32x4*>(out_s + pix * p.ldo + c0) = pk;
    }
}

// dtype and shape checks shared by the entry and mlpk_atm_sample_supported; fills the chunking
static int atm_geometry(int dtype, int B, int H, int W, int C, int share, AtmArgs* a) {
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || share <= 0) return MLPK_ESHAPE;
    if ((2LL * C) % share) return MLPK_ESHAPE;
    const int es = dtype == MLPK_F32 ? 4 : 2, epv = 16 / es;
    if (C % epv) return MLPK_ESHAPE;
    const long long lmax = H > W ? H : W;
    if (lmax * 16 > ATM_LDS_MAX) return MLPK_ESHAPE;                  // a line of one 16-byte channel vector must fit the LDS it is staged in
    int cc = 64;
    while (cc > epv && lmax * cc * es > ATM_LDS_MAX) cc >>= 1;
    a->B = B; a->H = H; a->W = W; a->C = C; a->share = share;
    a->cc = cc;
    a->nchunk = (C + cc - 1) / cc;
    if ((long long)B * (H + W) * a->nchunk > 0x7fffffffLL) return MLPK_ESHAPE;
    return 0;
}

template <typename T>
static int atm_launch(AtmArgs& a, void* stream) {
    const int ncol = a.out_h ? a.B * a.W * a.nchunk : 0;
    a.nrow = (a.out_w || a.out_c) ? a.B * a.H * a.nchunk : 0;
    const int lmax = a.H > a.W ? a.H : a.W;
    const int lds = lmax * a.cc * (int)sizeof(T);
    const dim3 grid((unsigned)(a.nrow + ncol));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    constexpr int EPV = 16 / (int)sizeof(T);
    if constexpr (EPV == 8) {
        if (a.share % 8 == 0) return launch_lds(atm_sample_kernel<T, 8>, grid, dim3(256), lds, s, a);
    }
    if (a.share % 4 == 0) return launch_lds(atm_sample_kernel<T, 4>, grid, dim3(256), lds, s, a);
    if (a.share % 2 == 0) return launch_lds(atm_sample_kernel<T, 2>, grid, dim3(256), lds, s, a);
    return launch_lds(atm_sample_kernel<T, 1>, grid, dim3(256), lds, s, a);
}

}  // namespace mlpk

using namespace mlpk;

extern "C" int mlpk_atm_tap(float off, int pos, int L, int* i0, int* i1, float* w0, float* w1) {
    if (!i0 || !i1 || !w0 || !w1) return MLPK_ENULL;
    if (L <= 0 || pos < 0 || pos >= L) return MLPK_ESHAPE;
    const AtmTap t = atm_tap(off, pos, L);
    *i0 = t.i0; *i1 = t.i1; *w0 = t.w0; *w1 = t.w1;
    return (t.ok0 ? 1 : 0) | (t.ok1 ? 2 : 0);
}

extern "C" int mlpk_atm_sample_supported(int dtype, int H, int W, int C, int share) {
    AtmArgs a;
    return atm_geometry(dtype, 1, H, W, C, share, &a) == 0;
}

extern "C" int mlpk_atm_sample(int dtype, const void* x, int64_t x_pitch, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, const void* off, int64_t off_pitch, int share, void* out_w, void* out_h, void* out_c,
                               int64_t out_pitch, int B, int H, int W, int C, void* stream) {
    if (!x || !off || (!out_w && !out_h && !out_c) || (mean != nullptr) != (rstd != nullptr)) return MLPK_ENULL;
    AtmArgs a;
    if (const int rc = atm_geometry(dtype, B, H, W, C, share, &a)) return rc;
    if (x_pitch < C || out_pitch < C || off_pitch < 2LL * C / share) return MLPK_ESHAPE;
    const int es = dtype == MLPK_F32 ? 4 : 2, epv = 16 / es;
    if (((uintptr_t)x & 15) || ((uintptr_t)out_w & 15) || ((uintptr_t)out_h & 15) || ((uintptr_t)out_c & 15) || x_pitch % epv || out_pitch % epv ||
        ((uintptr_t)off & (es - 1)))
        return MLPK_EALIGN;
    a.x = x; a.off = off; a.out_w = out_w; a.out_h = out_h; a.out_c = out_c;
    a.ldx = x_pitch; a.ldoff = off_pitch; a.ldo = out_pitch;
    a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
    switch (dtype) {
        case MLPK_F32: return atm_launch<float>(a, stream);
        case MLPK_F16: return atm_launch<f16_t>(a, stream);
        default: return atm_launch<bf16_t>(a, stream);
    }
}
