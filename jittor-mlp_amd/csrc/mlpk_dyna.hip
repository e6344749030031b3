// DynaMixer's dynamic token mixing (dyna_mlp.py:34-94, DynaMixerOp_w / DynaMixerOp_h), one axis per launch (mlpk.h mlpk_dyna_mix).  Per image,
// per line of L pixels along the axis and per channel segment g (s segments of d = C / s channels) the reference generates an L x L mixing matrix
// from the line itself -- logits z[l1 L + l2] = attend.1(v), v[l hd + j] = t[pix(l), g hd + j] -- takes the softmax over l2 and applies it to the
// segment's channels of LayerNorm(x) along the line.  Neither the logits nor LayerNorm(x) reach global memory:
//   a work item is one (line, segment); a workgroup takes DYNA_MB consecutive items, so the attend weight (shared by every item) is read once per
//   DYNA_MB items, whatever the numbers of lines and segments are (the last workgroup's missing items are skipped);
//   phase A   v of every item -> LDS, zero in the K padding (fp32: as fp32; 16-bit: in the storage type, 16 rows of K padded to 32);
//   phase B   logits, fp32 accumulation starting from the bias -> LDS [item][l1][l2].  16-bit types: on the matrix pipe (v_mfma_f32_16x16x32),
//             D[n][item] = A[n][k] v[item][k]: a lane's A fragment is ONE 16-byte load of the packed weight [k / e][n][e], its B fragment one LDS
//             read of v; half of the 16 item columns are padding.  fp32: thread n owns output column n (and n + 256, ...), one coalesced 16-byte
//             load of the packed weight serves e products of each item, v is an LDS broadcast read;
//   phase C   softmax over l2, four lanes per row (mlpk_dyna.h), the row maximum subtracted first, a true division for the reciprocal of the sum: a
//             one-hot row is exactly one-hot and a uniform row of a power-of-two L is exactly 1 / L;
//   phase D   per chunk of <= DYNA_DC channels of the segment: 16-byte loads of x, normalised in fp32 and rounded as mlpk_norm_apply does, staged in
//             LDS as [item][l][c]; then out[l1] = sum_l2 p[l1][l2] xn[l2] in fp32, four l1 per thread sharing each read of xn, one rounding, 16-byte stores.
// Everything an item reads or writes is its own: images, lines and segments do not see each other.
#include "mlpk_dyna.h"

namespace mlpk {

template <typename T> __device__ __forceinline__ f32x4 dyna_mfma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (dtype_of<T>::value == MLPK_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <typename T, int NB>
__global__ void __launch_bounds__(256) dyna_mix_kernel(const DynaArgs p) {
    constexpr int EPV = 16 / (int)sizeof(T);
    constexpr int MB = DYNA_MB;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int L = p.L, K = p.K, KP = p.KP, N = p.N, LP = p.LP;
    float* vs = reinterpret_cast<float*>(smem_raw);                   // [MB][KP]
    float* ps = vs + MB * KP;                                         // [MB][L][LP]
    T* xs = reinterpret_cast<T*>(ps + MB * L * LP);                   // [MB][L][dc]: dyna_softmax_mix's staging area
    const T* __restrict__ t = reinterpret_cast<const T*>(p.t);
    const T* __restrict__ aw = reinterpret_cast<const T*>(p.aw);
    const int tid = threadIdx.x;
    const int64_t item0 = (int64_t)blockIdx.x * MB;
    const int nitem = p.items - item0 < MB ? (int)(p.items - item0) : MB;         // >= 1 by the grid's size
    __shared__ int64_t ibase[DYNA_MB];
    __shared__ int ig[DYNA_MB];
    const int64_t step = p.axis == 0 ? p.W : 1;
    dyna_items(p, item0, nitem, tid, ibase, ig);
    __syncthreads();

    if constexpr (sizeof(T) == 2) {
        // phase A: v of every item -> LDS in the storage type (the values are t's own), [16][KP]: rows DYNA_MB .. 15 and the K padding are zero
        T* vt = reinterpret_cast<T*>(smem_raw);
        for (int idx = tid; idx < 16 * KP; idx += 256) {
            const int i = idx / KP, k = idx - i * KP;
            T val = from_f32<T>(0.0f);
            if (i < nitem && k < K) {
                const int64_t base = ibase[i];
                const int g = ig[i];
                const int l = k / p.hd, j = k - l * p.hd;
                val = t[(base + l * step) * p.ldt + p.toff + g * p.hd + j];
            }
            vt[idx] = val;
        }
        __syncthreads();

        // phase B: logits on the matrix pipe, D[n][item] = sum_k A[n][k] v[item][k] by v_mfma_f32_16x16x32: a wave owns 16 output columns n at a time.
        // Lane l holds A[n0 + (l & 15)][kb + 8 (l >> 4) + 0..7] -- ONE 16-byte load of the packed weight -- and v[item l & 15][the same k] from
        // LDS, and receives D[n0 + 4 (l >> 4) + 0..3][item l & 15]; fp32 accumulation starting from the bias.
        // A wave takes NB tiles at a time (tiles wave, wave + 4, ...: the four waves stay balanced for any N; NB = 2, 4 or 8, the smallest that
        // covers N in two rounds) and requests the weight fragments of all of them, for the next K step, before it multiplies the current ones:
        // NB loads in flight instead of a load -> multiply chain per tile.
        const int lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
        const int kgroups = p.KW / 8;
        auto load_a = [&](int kb, int nc) {
            const int kg = kb / 8 + kq;                               // K is padded to 32 for the instruction: the packed weight ends at K padded to 8
            const u32x4 a = *reinterpret_cast<const u32x4*>(aw + ((size_t)min(kg, kgroups - 1) * N + nc) * 8);
            return kg < kgroups ? a : u32x4{0u, 0u, 0u, 0u};
        };
        for (int t0 = 0; t0 * 16 < N; t0 += 4 * NB) {
            int n0[NB], nc[NB];
            f32x4 acc[NB];
            u32x4 a[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                n0[j] = (t0 + 4 * j + wave) * 16;
                nc[j] = min(n0[j] + col, N - 1);                      // (a row beyond N repeats row N - 1 and is not stored)
                a[j] = load_a(0, nc[j]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = p.ab[min(n0[j] + 4 * kq + i, N - 1)];
            }
            for (int kb = 0; kb < KP; kb += 32) {
                u32x4 an[NB];
                const int kn = min(kb + 32, KP - 32);                 // (the last step requests its own fragments again: no branch around the loads)
#pragma unroll
                for (int j = 0; j < NB; ++j) an[j] = load_a(kn, nc[j]);
                const u32x4 b = *reinterpret_cast<const u32x4*>(vt + col * KP + kb + 8 * kq);
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    acc[j] = dyna_mfma<T>(a[j], b, acc[j]);
                    a[j] = an[j];
                }
            }
            if (col < MB) {
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int nb = n0[j] + 4 * kq;                    // this lane's four rows nb .. nb + 3: ONE division per tile, then steps
                    int l1 = nb / L, l2 = nb - l1 * L;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (nb + i < N) ps[(col * L + l1) * LP + l2] = acc[j][i];
                        if (++l2 == L) { l2 = 0; ++l1; }
                    }
                }
            }
        }
    } else {
        // phase A: v
        for (int idx = tid; idx < MB * KP; idx += 256) {
            const int i = idx / KP, k = idx - i * KP;
            float val = 0.0f;
            if (i < nitem && k < K) {
                const int64_t base = ibase[i];
                const int g = ig[i];
                const int l = k / p.hd, j = k - l * p.hd;
                val = to_f32(t[(base + l * step) * p.ldt + p.toff + g * p.hd + j]);
            }
            vs[idx] = val;
        }
        __syncthreads();

        // phase B: logits
        for (int n0 = 0; n0 < N; n0 += 256 * NB) {
            int n[NB], nc[NB];
            float acc[NB][MB];
    #pragma unroll
            for (int j = 0; j < NB; ++j) {
                n[j] = n0 + j * 256 + tid;
                nc[j] = min(n[j], N - 1);                                 // (a lane beyond N computes column N - 1 again and stores nothing)
                const float b = p.ab[nc[j]];
    #pragma unroll
                for (int m = 0; m < MB; ++m) acc[j][m] = b;
            }
            for (int kc = 0; kc < KP / EPV; ++kc) {
                float w[NB][EPV];
    #pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const u32x4 raw = *reinterpret_cast<const u32x4*>(aw + ((size_t)kc * N + nc[j]) * EPV);
                    T e[EPV];
                    __builtin_memcpy(e, &raw, 16);
    #pragma unroll
                    for (int k = 0; k < EPV; ++k) w[j][k] = to_f32(e[k]);
                }
    #pragma unroll
                for (int m = 0; m < MB; ++m) {
                    float v[EPV];
    #pragma unroll
                    for (int k = 0; k < EPV; k += 4) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(vs + m * KP + kc * EPV + k);
                        v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
                    }
    #pragma unroll
                    for (int j = 0; j < NB; ++j)
    #pragma unroll
                        for (int k = 0; k < EPV; ++k) acc[j][m] = __builtin_fmaf(w[j][k], v[k], acc[j][m]);
                }
            }
    #pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (n[j] < N) {
                    const int l1 = n[j] / L, l2 = n[j] - l1 * L;
    #pragma unroll
                    for (int m = 0; m < MB; ++m) ps[(m * L + l1) * LP + l2] = acc[j][m];
                }
            }
        }
    }
    dyna_softmax_mix<T>(p, ps, xs, ibase, ig, nitem, tid);
}

template <typename T>
static int dyna_launch(const DynaArgs& a, void* stream) {
    const int lds = DYNA_MB * (a.KP + a.L * a.LP) * 4 + DYNA_MB * a.L * a.dc * (int)sizeof(T);
    const dim3 grid((unsigned)((a.items + DYNA_MB - 1) / DYNA_MB));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if constexpr (sizeof(T) == 2) {
        const int per_wave = ((a.N + 15) / 16 + 3) / 4;                    // 16-column tiles of the logits per wave
        if (per_wave > 4) return launch_lds(dyna_mix_kernel<T, 8>, grid, dim3(256), lds, s, a);
        if (per_wave > 2) return launch_lds(dyna_mix_kernel<T, 4>, grid, dim3(256), lds, s, a);
        return launch_lds(dyna_mix_kernel<T, 2>, grid, dim3(256), lds, s, a);
    } else {
        if (a.N > 512) return launch_lds(dyna_mix_kernel<T, 4>, grid, dim3(256), lds, s, a);
        if (a.N > 256) return launch_lds(dyna_mix_kernel<T, 2>, grid, dim3(256), lds, s, a);
        return launch_lds(dyna_mix_kernel<T, 1>, grid, dim3(256), lds, s, a);
    }
}

// ---- the unfused form: the logits come from memory (a GEMM wrote them), the softmax and the mix are dyna_softmax_mix as above
// v[item][l hd + j] = t[pix(l), toff + g hd + j], the GEMM's operand rows in item order; zeros in columns [K, kp).  One thread per (item, l).
template <typename T>
__global__ void __launch_bounds__(256) dyna_gather_kernel(const DynaArgs p, T* __restrict__ v, const int64_t ldv, const int kp) {
    const T* __restrict__ t = reinterpret_cast<const T*>(p.t);
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;             // < items L < 2^31 (checked by the entry)
    if (idx >= (unsigned)(p.items * p.L)) return;
    const unsigned item = idx / (unsigned)p.L, l = idx - item * (unsigned)p.L;
    const unsigned line = item / (unsigned)p.s, g = item - line * (unsigned)p.s;
    int64_t base, step;
    dyna_line(p, line, base, step);
    const T* src = t + (base + (int64_t)l * step) * p.ldt + p.toff + g * p.hd;
    T* dst = v + (int64_t)item * ldv + l * p.hd;
    for (int j = 0; j < p.hd; ++j) dst[j] = src[j];
    if (l == (unsigned)p.L - 1)
        for (int k = p.K; k < kp; ++k) v[(int64_t)item * ldv + k] = from_f32<T>(0.0f);
}

template <typename T>
__global__ void __launch_bounds__(256) dyna_from_logits_kernel(const DynaArgs p, const T* __restrict__ z, const int64_t ldz, const int vec) {
    constexpr int EPV = 16 / (int)sizeof(T);
    constexpr int MB = DYNA_MB;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int L = p.L, N = p.N, LP = p.LP;
    float* ps = reinterpret_cast<float*>(smem_raw);                   // [MB][L][LP]
    T* xs = reinterpret_cast<T*>(ps + MB * L * LP);                   // [MB][L][dc]
    const int tid = threadIdx.x;
    const int64_t item0 = (int64_t)blockIdx.x * MB;
    const int nitem = p.items - item0 < MB ? (int)(p.items - item0) : MB;
    __shared__ int64_t ibase[DYNA_MB];
    __shared__ int ig[DYNA_MB];
    dyna_items(p, item0, nitem, tid, ibase, ig);
    if (vec) {                                                        // 16-byte loads: N and the pitch are whole vectors, z is aligned
        const int nv = N / EPV;
        for (int idx = tid; idx < nitem * nv; idx += 256) {
            const int i = idx / nv, v = idx - i * nv;
            const u32x4 raw = *reinterpret_cast<const u32x4*>(z + (item0 + i) * ldz + v * EPV);
            T e[EPV];
            __builtin_memcpy(e, &raw, 16);
            int l1 = (v * EPV) / L, l2 = v * EPV - l1 * L;
#pragma unroll
            for (int k = 0; k < EPV; ++k) {
                ps[(i * L + l1) * LP + l2] = to_f32(e[k]);
                if (++l2 == L) { l2 = 0; ++l1; }
            }
        }
    } else {
        for (int idx = tid; idx < nitem * N; idx += 256) {
            const int i = idx / N, n = idx - i * N;
            const int l1 = n / L, l2 = n - l1 * L;
            ps[(i * L + l1) * LP + l2] = to_f32(z[(item0 + i) * ldz + n]);
        }
    }
    dyna_softmax_mix<T>(p, ps, xs, ibase, ig, nitem, tid);
}

template <typename T>
static int dyna_gather_launch(const DynaArgs& a, void* v, int64_t ldv, int kp, void* stream) {
    const dim3 grid((unsigned)((a.items * a.L + 255) / 256));
    hipLaunchKernelGGL((dyna_gather_kernel<T>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, reinterpret_cast<T*>(v), ldv, kp);
    return (int)hipGetLastError();
}

template <typename T>
static int dyna_from_logits_launch(const DynaArgs& a, const void* z, int64_t ldz, void* stream) {
    constexpr int EPV = 16 / (int)sizeof(T);
    const int lds = DYNA_MB * a.L * a.LP * 4 + DYNA_MB * a.L * a.dc * (int)sizeof(T);
    const dim3 grid((unsigned)((a.items + DYNA_MB - 1) / DYNA_MB));
    const int vec = a.N % EPV == 0 && ldz % EPV == 0 && ((uintptr_t)z & 15) == 0;
    return launch_lds(dyna_from_logits_kernel<T>, grid, dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a, reinterpret_cast<const T*>(z), ldz, vec);
}

}  // namespace mlpk

using namespace mlpk;

extern "C" int mlpk_dyna_mix_supported(int dtype, int L, int C, int s, int hd) {
    DynaArgs a;
    return dyna_geometry(dtype, L, C, s, hd, &a) == 0;
}

extern "C" int mlpk_dyna_mix(int dtype, const void* x, int64_t x_pitch, const float* mean, const float* rstd, const float* gamma, const float* beta,
                             const void* t, int64_t t_pitch, int t_off, const void* aw, const float* ab, void* out, int64_t out_pitch, int B, int H,
                             int W, int C, int s, int hd, int axis, void* stream) {
    if (!x || !t || !aw || !ab || !out || (mean != nullptr) != (rstd != nullptr)) return MLPK_ENULL;
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (B <= 0 || H <= 0 || W <= 0 || (axis != 0 && axis != 1)) return MLPK_ESHAPE;
    DynaArgs a;
    if (const int rc = dyna_geometry(dtype, axis ? W : H, C, s, hd, &a)) return rc;
    if (x_pitch < C || out_pitch < C || t_off < 0 || t_pitch < (int64_t)t_off + (int64_t)s * hd) return MLPK_ESHAPE;
    a.Q = axis ? H : W;
    a.items = (int64_t)B * a.Q * s;
    if ((a.items + DYNA_MB - 1) / DYNA_MB > 0x7fffffffLL) return MLPK_ESHAPE;
    const int es = dtype == MLPK_F32 ? 4 : 2, epv = 16 / es;
    if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) || ((uintptr_t)aw & 15) || x_pitch % epv || out_pitch % epv || ((uintptr_t)t & (es - 1)) ||
        ((uintptr_t)ab & 3))
        return MLPK_EALIGN;
    a.x = x; a.t = t; a.aw = aw; a.ab = ab; a.out = out;
    a.ldx = x_pitch; a.ldt = t_pitch; a.ldo = out_pitch;
    a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
    a.toff = t_off; a.H = H; a.W = W; a.axis = axis;
    switch (dtype) {
        case MLPK_F32: return dyna_launch<float>(a, stream);
        case MLPK_F16: return dyna_launch<f16_t>(a, stream);
        default: return dyna_launch<bf16_t>(a, stream);
    }
}

extern "C" int mlpk_dyna_gather(int dtype, const void* t, int64_t t_pitch, int t_off, void* v, int64_t v_pitch, int kp, int B, int H, int W, int s, int hd,
                                int axis, void* stream) {
    if (!t || !v) return MLPK_ENULL;
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (B <= 0 || H <= 0 || W <= 0 || s <= 0 || hd <= 0 || (axis != 0 && axis != 1)) return MLPK_ESHAPE;
    const int L = axis ? W : H;
    if (L > DYNA_LMAX || (long long)L * hd > DYNA_KMAX) return MLPK_ESHAPE;
    if (kp < L * hd || v_pitch < kp || t_off < 0 || t_pitch < (int64_t)t_off + (int64_t)s * hd) return MLPK_ESHAPE;
    DynaArgs a = {};
    a.L = L; a.s = s; a.hd = hd; a.K = L * hd; a.Q = axis ? H : W; a.H = H; a.W = W; a.axis = axis;
    a.items = (int64_t)B * a.Q * s;
    if (a.items * L > 0x7fffffffLL) return MLPK_ESHAPE;
    const int es = dtype == MLPK_F32 ? 4 : 2;
    if (((uintptr_t)t & (es - 1)) || ((uintptr_t)v & (es - 1))) return MLPK_EALIGN;
    a.t = t; a.ldt = t_pitch; a.toff = t_off;
    switch (dtype) {
        case MLPK_F32: return dyna_gather_launch<float>(a, v, v_pitch, kp, stream);
        case MLPK_F16: return dyna_gather_launch<f16_t>(a, v, v_pitch, kp, stream);
        default: return dyna_gather_launch<bf16_t>(a, v, v_pitch, kp, stream);
    }
}

extern "C" int mlpk_dyna_mix_logits(int dtype, const void* x, int64_t x_pitch, const float* mean, const float* rstd, const float* gamma,
                                    const float* beta, const void* z, int64_t z_pitch, void* out, int64_t out_pitch, int B, int H, int W, int C, int s,
                                    int hd, int axis, void* stream) {
    if (!x || !z || !out || (mean != nullptr) != (rstd != nullptr)) return MLPK_ENULL;
    if (dtype != MLPK_F32 && dtype != MLPK_F16 && dtype != MLPK_BF16) return MLPK_EDTYPE;
    if (B <= 0 || H <= 0 || W <= 0 || (axis != 0 && axis != 1)) return MLPK_ESHAPE;
    DynaArgs a;
    if (const int rc = dyna_geometry(dtype, axis ? W : H, C, s, hd, &a)) return rc;
    if (x_pitch < C || out_pitch < C || z_pitch < a.N) return MLPK_ESHAPE;
    a.Q = axis ? H : W;
    a.items = (int64_t)B * a.Q * s;
    if ((a.items + DYNA_MB - 1) / DYNA_MB > 0x7fffffffLL) return MLPK_ESHAPE;
    const int es = dtype == MLPK_F32 ? 4 : 2, epv = 16 / es;
    if (((uintptr_t)x & 15) || ((uintptr_t)out & 15) || x_pitch % epv || out_pitch % epv || ((uintptr_t)z & (es - 1))) return MLPK_EALIGN;
    a.x = x; a.t = nullptr; a.aw = nullptr; a.ab = nullptr; a.out = out;
    a.ldx = x_pitch; a.ldt = 0; a.ldo = out_pitch;
    a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
    a.toff = 0; a.H = H; a.W = W; a.axis = axis;
    switch (dtype) {
        case MLPK_F32: return dyna_from_logits_launch<float>(a, z, z_pitch, stream);
        case MLPK_F16: return dyna_from_logits_launch<f16_t>(a, z, z_pitch, stream);
        default: return dyna_from_logits_launch<bf16_t>(a, z, z_pitch, stream);
    }
}
