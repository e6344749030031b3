// What the fused mlpk_dyna_mix and the unfused mlpk_dyna_gather / mlpk_dyna_mix_logits (all in mlpk_dyna.hip) share: the argument block, the
// shape checks, and the softmax-and-mix phases as device code.
#pragma once
#include "mlpk_common.h"


namespace mlpk {

constexpr int DYNA_MB = 8;        // items per workgroup
constexpr int DYNA_LMAX = 32;
constexpr int DYNA_KMAX = 256;    // L hd
constexpr int DYNA_DC = 32;       // channels of a segment staged at a time
constexpr int DYNA_R = 4;         // rows l1 per thread in phase D

struct DynaArgs {
    const void* x;
    const void* t;
    const void* aw;      // [KP / e][N][e], e = elements per 16 bytes
    const float* ab;     // [N]
    void* out;
    int64_t ldx, ldt, ldo;
    const float* mean;   // per pixel, or NULL: 0 / 1
    const float* rstd;
    const float* gamma;  // per channel, or NULL: 1
    const float* beta;   // or NULL: 0
    int toff;
    int H, W, s, hd, axis;
    int L, Q, d, K, KW, KP, N, LP, dc;   // KW: K padded to e (the packed weight); KP: v's LDS row (16-bit: K padded to 32, the MFMA's K step)
    int64_t items;       // B Q s
};

// (mlpk_raft.hip raft_f32: keeps the fp32 result a value of its own, so that fma + conversion are not fused into one rounding and xn has
// mlpk_norm_apply's bits)
__device__ __forceinline__ float dyna_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xE4, 0xF, 0xF, false));
}

// maximum over each group of 4 consecutive lanes, in every lane of the group (quad_sum's two steps with fmaxf)
__device__ __forceinline__ float dyna_quad_max(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
    return v;
}

// the first pixel of an item's line and the distance between neighbours on it (axis 0: a column, L = H; axis 1: a row, L = W)
__device__ __forceinline__ void dyna_line(const DynaArgs& p, int64_t line, int64_t& base, int64_t& step) {
    const int64_t b = line / p.Q, q = line - b * p.Q;
    if (p.axis == 0) { base = b * p.H * p.W + q; step = p.W; }
    else { base = (b * p.H + q) * p.W; step = 1; }
}

// The geometry of a workgroup's items, worked out once by its first DYNA_MB threads (the 64-bit divisions are slow: no other phase divides by s or
// Q): ibase[i] = the first pixel of item i's line, ig[i] = its segment.  The caller synchronises before it reads them.
__device__ __forceinline__ void dyna_items(const DynaArgs& p, const int64_t item0, const int nitem, const int tid, int64_t* ibase, int* ig) {
    if (tid < DYNA_MB) {
        const int64_t item = item0 + (tid < nitem ? tid : 0);
        const int64_t line = item / p.s;
        int64_t base, step;
        dyna_line(p, line, base, step);
        ibase[tid] = base;
        ig[tid] = (int)(item - line * p.s);
    }
}

// phases C and D for the items [item0, item0 + nitem) whose logits lie in ps [item][l1][LP]: the softmax over l2, then the mix of LayerNorm(x), a chunk of
// the segment's channels at a time through xs [item][l][dc].  ibase / ig: dyna_items' tables.  The caller has not synchronised yet.  (Its own function: the fused kernel and the
// unfused form, which reads the logits from memory, run the same device code.)
template <typename T>
__device__ __forceinline__ void dyna_softmax_mix(const DynaArgs& p, float* ps, T* xs, const int64_t* ibase, const int* ig, const int nitem, const int tid) {
    constexpr int EPV = 16 / (int)sizeof(T);
    constexpr int MB = DYNA_MB;
    const int L = p.L, LP = p.LP, dc = p.dc;
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    T* out = reinterpret_cast<T*>(p.out);
    const int64_t step = p.axis == 0 ? p.W : 1;
    __syncthreads();                                                  // the logits are complete

    // phase C: softmax over l2, four adjacent lanes per row (elements q, q + 4, ...), maximum and sum combined across the quad by DPP
    for (int r = tid >> 2; r < nitem * L; r += 64) {                     // (r is the same in the four lanes of a quad: all of them are active)
        float* row = ps + r * LP;
        const int q = tid & 3;
        float mx = -__builtin_inff();
        for (int l2 = q; l2 < L; l2 += 4) mx = fmaxf(mx, row[l2]);
        mx = dyna_quad_max(mx);
        float sum = 0.0f;
        for (int l2 = q; l2 < L; l2 += 4) {
            const float e = __expf(row[l2] - mx);
            row[l2] = e;
            sum += e;
        }
        const float inv = 1.0f / quad_sum(sum);                       // a true division: exactly 1 for a one-hot row, exactly 1 / L for L equal logits, L a power of two
        for (int l2 = q; l2 < L; l2 += 4) row[l2] *= inv;
    }

    // phase D: the mix, a chunk of the segment's channels at a time
    const int LG = (L + DYNA_R - 1) / DYNA_R;
    for (int c0 = 0; c0 < p.d; c0 += dc) {
        const int nv = min(dc, p.d - c0) / EPV;
        __syncthreads();                                              // the softmax is complete / the previous chunk has been read
        for (int u = tid; u < nitem * L * nv; u += 256) {
            const int v = u % nv, r = u / nv;
            const int l = r % L, i = r / L;
            const int64_t base = ibase[i];
            const int g = ig[i];
            const int64_t pix = base + l * step;
            const int c = g * p.d + c0 + v * EPV;
            const u32x4 raw = *reinterpret_cast<const u32x4*>(x + pix * p.ldx + c);
            float mu = 0.f, rs = 1.f;
            if (p.mean) { mu = p.mean[pix]; rs = p.rstd[pix]; }
            T a[EPV], e[EPV];
            __builtin_memcpy(a, &raw, 16);
#pragma unroll
            for (int k = 0; k < EPV; ++k) {
                const float gm = p.gamma ? p.gamma[c + k] : 1.0f;
                const float bt = p.beta ? p.beta[c + k] : 0.0f;
                e[k] = from_f32<T>(dyna_f32(__builtin_fmaf((to_f32(a[k]) - mu) * rs, gm, bt)));   // (norm_apply_tile_kernel's form)
            }
            u32x4 pk;
            __builtin_memcpy(&pk, e, 16);
            *reinterpret_cast<u32x4*>(xs + (size_t)(i * L + l) * dc + v * EPV) = pk;
        }
        __syncthreads();
        for (int u = tid; u < nitem * LG * nv; u += 256) {
            const int v = u % nv, r = u / nv;
            const int lg = r % LG, i = r / LG;
            const int l10 = lg * DYNA_R;
            const float* prow[DYNA_R];
#pragma unroll
            for (int a = 0; a < DYNA_R; ++a) prow[a] = ps + (i * L + min(l10 + a, L - 1)) * LP;      // (rows beyond L repeat row L - 1 and are not stored)
            float acc[DYNA_R][EPV];
#pragma unroll
            for (int a = 0; a < DYNA_R; ++a)
#pragma unroll
                for (int k = 0; k < EPV; ++k) acc[a][k] = 0.0f;
            const T* col = xs + (size_t)i * L * dc + v * EPV;
            for (int l2 = 0; l2 < L; ++l2) {
                const u32x4 raw = *reinterpret_cast<const u32x4*>(col + (size_t)l2 * dc);
                T e[EPV];
                __builtin_memcpy(e, &raw, 16);
                float xv[EPV];
#pragma unroll
                for (int k = 0; k < EPV; ++k) xv[k] = to_f32(e[k]);
#pragma unroll
                for (int a = 0; a < DYNA_R; ++a) {
                    const float w = prow[a][l2];
#pragma unroll
                    for (int k = 0; k < EPV; ++k) acc[a][k] = __builtin_fmaf(w, xv[k], acc[a][k]);
                }
            }
            const int64_t base = ibase[i];
            const int g = ig[i];
            const int c = g * p.d + c0 + v * EPV;
#pragma unroll
            for (int a = 0; a < DYNA_R; ++a) {
                if (l10 + a < L) {
                    T e[EPV];
#pragma unroll
                    for (int k = 0; k < EPV; ++k) e[k] = from_f32<T>(acc[a][k]);
                    u32x4 pk;
                    __builtin_memcpy(&pk, e, 16);
                    *reinterpret_cast<u32x4*>(out + (base + (int64_t)(l10 + a) * step) * p.ldo + c) = pk;
                }
            }
        }
    }
}

// dtype and shape checks shared by the entry and mlpk_dyna_mix_supported; fills the derived sizes
static inline int dyna_geometry(int dtype, int L, int C, int s, int hd, DynaArgs* a) {
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (L <= 0 || C <= 0 || s <= 0 || hd <= 0) return MLPK_ESHAPE;
    if (L > DYNA_LMAX || (long long)L * hd > DYNA_KMAX || C % s) return MLPK_ESHAPE;
    const int epv = dtype == MLPK_F32 ? 4 : 8;
    const int d = C / s;
    if (d % epv) return MLPK_ESHAPE;
    a->L = L; a->s = s; a->hd = hd; a->d = d;
    a->K = L * hd;
    a->KW = (a->K + epv - 1) / epv * epv;
    a->KP = dtype == MLPK_F32 ? a->KW : (a->K + 31) / 32 * 32;
    a->N = L * L;
    a->LP = L | 1;
    a->dc = d < DYNA_DC ? d : DYNA_DC;
    return 0;
}

}  // namespace mlpk
