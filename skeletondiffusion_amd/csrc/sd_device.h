// What every kernel translation unit here spells the same way: the LDS limits of a CU and the opt-in
// to a large dynamic allocation, the vector types, and the few one-line device helpers.
//
// The limits are plain C++ (tests/host/gl4_lds_check.cpp reads them through sd_gl4_lds.h); everything
// else needs hipcc.
#pragma once
#include <stddef.h>

namespace sd {

constexpr size_t kLdsDefault = 64 * 1024;  // dynamic LDS a launch may take without the attribute call
constexpr size_t kLdsMax = 160 * 1024;     // of a CU: a launcher refuses a larger tile, with its own error code

}  // namespace sd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace sd {

// Opts `kernel` into `lds` bytes of dynamic LDS where the default does not cover them.  The caller has
// already refused lds > kLdsMax.
template <class Kernel>
inline hipError_t lds_opt_in(Kernel kernel, size_t lds) {
    if (lds <= kLdsDefault) return hipSuccess;
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// the destination type of __builtin_amdgcn_global_load_lds (LDS-DMA)
typedef __attribute__((address_space(3))) void lds_void;

// s_waitcnt immediate for "vmcnt <= N" with lgkmcnt / expcnt not waited (gfx9 encoding:
// vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt_hi[15:14])
template <int N>
struct VmCnt {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    static constexpr int imm = (N & 0xF) | (0x7 << 4) | (0xF << 8) | ((N >> 4) << 14);
};

// 16 aligned bytes from global memory or LDS (the compiler picks the instruction from the address)
__device__ __forceinline__ floatx4 ld4(const float* p) { return *reinterpret_cast<const floatx4*>(p); }

__device__ __forceinline__ floatx4 mfma4(float a, float b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

}  // namespace sd
#endif
