// Stand-in for <hip/hip_runtime.h> when the device-side arithmetic headers of nfllib_amd/csrc (modarith.h, dot_reduce.h,
// baseconv_pos.h) are compiled for the CPU by tests/cpp_baseconv/baseconv_pos_main.cpp: the qualifiers vanish and the two
// high-multiply intrinsics are written with a double-width product.  Nothing else of the runtime is needed by those headers.
#pragma once
#include <stdint.h>
#define __device__
#define __host__
#define __forceinline__ inline
static inline uint64_t __umul64hi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
#ifndef __clang__
#define __builtin_nondeterministic_value(x) (x)
#endif
