// The two taps of ActiveMLP's 1-D sampling (mlpk.h mlpk_atm_sample): torchvision's deform_conv2d bilinear rule with one of (dy, dx) identically
// zero.  ONE source expression for the kernel (device) and for mlpk_atm_tap (host), so that what a CPU test proves about NaN, +-inf, huge
// offsets and the boundaries -1, L - 1, L holds for the kernel's address arithmetic too.
#pragma once
#include <hip/hip_runtime.h>

namespace mlpk {

struct AtmTap {
    int i0, i1;      // source positions, each inside [0, L - 1] (0 where its flag is clear: never an unchecked index)
    float w0, w1;    // 1 - f and f, f = p - floor(p); both 0 outside the map
    bool ok0, ok1;   // whether the tap contributes
};

// position p = pos + off on an axis of L pixels.  The sample is 0 unless -1 < p < L; "inside" is decided by FLOAT comparisons, which are
// false for NaN and settle +-inf and offsets beyond the int range, before anything is converted to an integer: floor(p) then lies in
// [-1, L - 1], exactly representable.
__host__ __device__ inline AtmTap atm_tap(float off, int pos, int L) {
    AtmTap t = {0, 0, 0.0f, 0.0f, false, false};
    const float p = (float)pos + off;
    if (!(p > -1.0f && p < (float)L)) return t;
    const float fl = __builtin_floorf(p);
    const float f = p - fl;
    const int i = (int)fl;
    t.w0 = 1.0f - f;
    t.w1 = f;
    t.ok0 = i >= 0 && i <= L - 1;
    t.ok1 = i + 1 >= 0 && i + 1 <= L - 1;
    t.i0 = t.ok0 ? i : 0;
    t.i1 = t.ok1 ? i + 1 : 0;
    return t;
}

}  // namespace mlpk
