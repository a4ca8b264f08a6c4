// The law of an fp16 scale slot {scale, floor, running |max|} (c16.hpp, ebfi_amd/f16scale.py), stated ONCE for the device
// kernels (ScaleSlot::record, pack_table_f16_kernel, f16_scales_finish_kernel) and for host programs (oracle/scale_law_host.cpp;
// f16scale.next_scale and oracle/scale_ref.py restate it and are pinned against it bit for bit).  Plain C++: no HIP include, no
// memory access -- the callers load the slot's words and store the results.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define EBFI_LAW_FN __host__ __device__ inline
#else
#define EBFI_LAW_FN inline
#endif

namespace ebfi {

constexpr int F16_TARGET_EXP = 2;          // next scale: |max| * scale in [2^(F16_TARGET_EXP-1), 2^F16_TARGET_EXP) (f16scale.TARGET_EXP)
constexpr int F16_SCALE_EXP_MAX = 120;     // ... but never above 2^120: a |max| below 2^-118 keeps that scale (the x0.1
                                           // initialisation does produce 1e-29 gradients; 2 - e reaches 150 for a subnormal)
constexpr float F16_AMAX_LIMIT = 3.0e38f;  // a recorded |max| above this (+inf and NaN included) is "not finite"
constexpr float F16_RANGE_LIMIT = 60000.f; // |max| * scale-in-use above this could have left fp16's range (65504)
constexpr float F16_FLOOR_FACTOR = 0.875f; // next step's floor: only waves above 7/8 of this step's maximum report

struct SlotUpdate {
    float scale, floor;                    // the slot's words [0] and [SLOT_FLOOR] after the finish launch ([SLOT_AMAX] is always 0)
    int flag;                              // 1: the step's gradients are suspect (or'ed into guard[0])
};

// One slot of the finish launch: a = recorded |max|, s = scale in use, floor = floor in use.
EBFI_LAW_FN SlotUpdate finish_slot(float a, float s, float floor) {
    if (!(a > 0.f))                        // nothing staged through this slot, or nothing above the floor: keep the scale;
        return {s, floor * 0.5f, a != a ? 1 : 0};   // the floor decays fast (a tensor that shrank is measured again within a few steps)
    const int flag = (!(a <= F16_AMAX_LIMIT) || a * s > F16_RANGE_LIMIT) ? 1 : 0;
    if (!(a <= F16_AMAX_LIMIT)) return {s, 0.f, flag};
    int e;
    (void)frexpf(a, &e);                   // a = m * 2^e, m in [0.5, 1)
    const int k = F16_TARGET_EXP - e;
    return {ldexpf(1.f, k < F16_SCALE_EXP_MAX ? k : F16_SCALE_EXP_MAX), F16_FLOOR_FACTOR * a, flag};
}

// Whether a wave whose own maximum is m sends its atomic, given the slot's running |max| and floor as it reads them: only a value
// above both needs it; NaN compares false and goes through.
EBFI_LAW_FN bool should_report(float m, float amax_now, float floor) { return !(m <= fmaxf(amax_now, floor)); }

}  // namespace ebfi
