// What every disc*.hip needs, local to the translation unit that includes it.
#pragma once
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

using mrefsr::grid_of;

__device__ inline float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

}  // namespace
