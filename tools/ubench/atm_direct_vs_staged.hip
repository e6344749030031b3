// mlpk_atm_sample (the line staged in LDS) against a direct-global version of the same sampling: bf16, batch 256, the four stage shapes of ActiveTiny.
// Prints one JSON line per shape (time per call by HIP events over 50 calls, effective TB/s = one read of x and of the offsets + three writes) and
// the number of output elements whose bits differ between the two.  The measurement behind README.md's ActiveMLP bullet (profiles/active_atm_direct_vs_staged.jsonl).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/atm_direct_vs_staged.hip -o atm_direct_vs_staged.bin -Ljittor-mlp_amd/lib -lmlpk -Wl,-rpath,$PWD/jittor-mlp_amd/lib
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../jittor-mlp_amd/csrc/mlpk_atm_tap.h"
#include "../../include/mlpk.h"

typedef __bf16 T;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("hip error %d at line %d\n", (int)e, __LINE__); exit(1); } } while (0)

__device__ __forceinline__ float keep(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xE4, 0xF, 0xF, false));
}

__global__ void __launch_bounds__(256) direct_kernel(const T* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, const T* __restrict__ off, int share,
                                                     T* out_w, T* out_h, T* out_c, int B, int H, int W, int C) {
    const int nv = C / 8;
    const int64_t total = (int64_t)B * H * W * nv;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t pix = i / nv;
    const int v = (int)(i - pix * nv), c0 = v * 8;
    const int xw = (int)(pix % W), yh = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    const int n_off = 2 * C / share;
    auto norm = [&](int64_t q, int c) -> float {
        return (float)(T)keep(__builtin_fmaf(((float)x[q * C + c] - mean[q]) * rstd[q], gamma[c], beta[c]));
    };
    T ec[8], ew[8], eh[8];
    for (int k = 0; k < 8; ++k) {
        const int c = c0 + k;
        ec[k] = (T)norm(pix, c);
        {
            const mlpk::AtmTap t = mlpk::atm_tap((float)off[pix * n_off + c / share], xw, W);
            float r = 0.f;
            if (t.ok0) r = t.w0 * norm((b * H + yh) * W + t.i0, c);
            if (t.ok1 && t.w1 != 0.f) r = __builtin_fmaf(t.w1, norm((b * H + yh) * W + t.i1, c), r);
            ew[k] = (T)r;
        }
        {
            const mlpk::AtmTap t = mlpk::atm_tap((float)off[pix * n_off + (C + c) / share], yh, H);
            float r = 0.f;
            if (t.ok0) r = t.w0 * norm((b * H + t.i0) * W + xw, c);
            if (t.ok1 && t.w1 != 0.f) r = __builtin_fmaf(t.w1, norm((b * H + t.i1) * W + xw, c), r);
            eh[k] = (T)r;
        }
    }
    *reinterpret_cast<u32x4*>(out_c + pix * C + c0) = *reinterpret_cast<const u32x4*>(ec);
    *reinterpret_cast<u32x4*>(out_w + pix * C + c0) = *reinterpret_cast<const u32x4*>(ew);
    *reinterpret_cast<u32x4*>(out_h + pix * C + c0) = *reinterpret_cast<const u32x4*>(eh);
}

int main() {
    const int B = 256;
    const int shapes[4][3] = {{56, 64, 2}, {28, 128, 4}, {14, 320, 4}, {7, 512, 8}};
    for (auto& s : shapes) {
        const int S = s[0], C = s[1], share = s[2];
        const int64_t rows = (int64_t)B * S * S, n_off = 2 * C / share;
        std::vector<T> hx(rows * C), ho(rows * n_off);
        std::vector<float> hm(rows, 0.1f), hr(rows, 1.5f), hg(C, 1.25f), hb(C, 0.5f);
        uint32_t st = 12345;
        auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)(st >> 8) / 16777216.0f; };
        for (auto& e : hx) e = (T)(rnd() * 4.f - 2.f);
        for (auto& e : ho) e = (T)(rnd() * 6.f - 3.f);
        T *x, *off, *o[6];
        float *m, *r, *g, *bt;
        CK(hipMalloc(&x, rows * C * 2)); CK(hipMalloc(&off, rows * n_off * 2));
        for (auto& p : o) CK(hipMalloc(&p, rows * C * 2));
        CK(hipMalloc(&m, rows * 4)); CK(hipMalloc(&r, rows * 4)); CK(hipMalloc(&g, C * 4)); CK(hipMalloc(&bt, C * 4));
        CK(hipMemcpy(x, hx.data(), rows * C * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(off, ho.data(), rows * n_off * 2, hipMemcpyHostToDevice));
        CK(hipMemcpy(m, hm.data(), rows * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(r, hr.data(), rows * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(g, hg.data(), C * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(bt, hb.data(), C * 4, hipMemcpyHostToDevice));
        const int64_t total = rows * (C / 8);
        auto direct = [&]() { hipLaunchKernelGGL(direct_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, x, m, r, g, bt, off, share, o[0], o[1], o[2], B, S, S, C); };
        auto staged = [&]() { if (mlpk_atm_sample(MLPK_BF16, x, C, m, r, g, bt, off, n_off, share, o[3], o[4], o[5], C, B, S, S, C, nullptr)) { printf("staged refused\n"); exit(1); } };
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        float ms[2];
        for (int which = 0; which < 2; ++which) {
            for (int i = 0; i < 5; ++i) which ? staged() : direct();
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(e0));
            for (int i = 0; i < 50; ++i) which ? staged() : direct();
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms[which], e0, e1));
        }
        std::vector<T> a(rows * C), bb(rows * C);
        int64_t diff = 0;
        for (int k = 0; k < 3; ++k) {
            CK(hipMemcpy(a.data(), o[k], rows * C * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(bb.data(), o[3 + k], rows * C * 2, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < rows * C; ++i) diff += __builtin_memcmp(&a[i], &bb[i], 2) != 0;
        }
        const double bytes = (double)(rows * C * 4 + rows * n_off) * 2;
        printf("{\"map\": %d, \"C\": %d, \"share\": %d, \"direct_us\": %.2f, \"staged_us\": %.2f, \"direct_TBps\": %.3f, \"staged_TBps\": %.3f, \"elements_differing\": %lld}\n",
               S, C, share, ms[0] * 20.0, ms[1] * 20.0, bytes / (ms[0] / 50 * 1e-3) * 1e-12, bytes / (ms[1] / 50 * 1e-3) * 1e-12, (long long)diff);
        CK(hipFree(x)); CK(hipFree(off)); for (auto& p : o) CK(hipFree(p));
        CK(hipFree(m)); CK(hipFree(r)); CK(hipFree(g)); CK(hipFree(bt));
    }
    return 0;
}
