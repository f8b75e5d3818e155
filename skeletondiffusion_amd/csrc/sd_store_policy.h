// One 16-B global store with a cache policy.
//
// The XCD L2s are write-back and not coherent with each other, so whatever a kernel has dirtied by
// plain stores is written back behind its last wave, before a dependent kernel may start.  A store with
// the sc1 bit writes through (the bytes leave L2 while the kernel is still running) and drops the line,
// so the end of the kernel finds it clean.
//
// Only for sites where ONE store instruction of one wave writes whole 128-B lines (the GEMM phase's
// scratch blocks, sd_ystore_map.h: one contiguous KiB per instruction).  A write-through store of part
// of a line is a fabric write of its own per part; such sites stay plain.
//
// POLICY 1 is inline asm.  The compiler's tracked form with this bit is the raw buffer store builtin
// (__builtin_amdgcn_raw_buffer_store_b128, aux 16: buffer_store_dwordx4 ... sc1); it is not used because
// the ISA guards of k_gl4t's store tail (tests/test_isa_waits.py, tests/test_isa_direct_y_store.py) count
// global_store instructions there (DESIGN.md §4ab has its measurement).  What the asm owes, by hand:
//   * wait states: the string ends with s_nop 1, the two wait states a VALU write to the data registers
//     needs behind a dwordx4 store (the compiler pads nothing behind asm);
//   * vmcnt: the waitcnt pass does not count these stores.  vmcnt returns in issue order on gfx9, so an
//     uncounted store makes a later counted wait stricter, never looser;
//   * order: volatile asm keeps program order among such stores (two from one lane to one address: the
//     second wins); no memory clobber is named, so plain global accesses may move across one -- only for
//     destinations the kernel does not read;
//   * LDS: the compiler moves no LDS read across volatile asm.  What feeds the NEXT store from LDS is read,
//     in the source, before this one.
#pragma once
#include "sd_device.h"

namespace sd {

constexpr int kStorePlain = 0;         // write-back: the line stays, dirty, in the XCD's L2
constexpr int kStoreWriteThrough = 1;  // sc1: written through, the line dropped

// the policy of each store class; the classes not listed here are plain stores in their kernels
constexpr int kStoreGemmY = kStoreWriteThrough;  // GEMM-phase Y into the row-blocked scratch (k_gl4t, k_gl4y)

// p + BYTE_OFF: an immediate of the instruction (-4096 .. 4095), so constant pieces of a tile cost no
// address arithmetic
template <int POLICY, int BYTE_OFF = 0>
__device__ __forceinline__ void store16(float* p, floatx4 v) {
    static_assert(POLICY == kStorePlain || POLICY == kStoreWriteThrough, "store policy");
    static_assert(BYTE_OFF >= -4096 && BYTE_OFF < 4096 && BYTE_OFF % 16 == 0, "immediate offset");
    if constexpr (POLICY == kStoreWriteThrough)
        asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1\n\ts_nop 1" ::"v"(p), "v"(v), "n"(BYTE_OFF));
    else
        *reinterpret_cast<floatx4*>(reinterpret_cast<char*>(p) + BYTE_OFF) = v;
}

}  // namespace sd
