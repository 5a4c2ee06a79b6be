// sample_u8.hpp -- one sample of an image as a byte, for the kernels that take a uint8 or a float32 frame in its own strides (the JPEG
// encoder's first stage, jpeg.hip; the re-distortion's taps, redistort.hip).  float32 goes through the presented frame's conversion
// (mtgs_present.h): NaN -> 0, clamp to [0, 1], times 255, with `round` plus 0.5, truncated.
#pragma once
#include "common.hpp"

__device__ __forceinline__ int load_sample(const void *image, bool is_float, bool round, int64_t at) {
    if (!is_float) return ((const uint8_t *)image)[at];
    float x = ((const float *)image)[at];
    x = x != x ? 0.f : (x < 0.f ? 0.f : (x > 1.f ? 1.f : x));
    x = __fmul_rn(x, 255.f);                 // two roundings, as mtgs_present.h's formats: never one fused multiply-add
    if (round) x = __fadd_rn(x, 0.5f);
    return (int)(uint32_t)x;
}
