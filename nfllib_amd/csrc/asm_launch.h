// asm_launch.h -- internal: what the dispatch of kernels_fast.hip needs of asm_launch.hip beyond kernels.h
#pragma once
#include "kernels.h"

namespace nflhip {

static constexpr int kLogN = 12;      // the 4096-word block of the 64-bit kernels ...
static constexpr int kThreads = 256;  // ... and its workgroup

enum AsmKind {
#define X(kind, name, row, level, whole) kind,
#include "asm_kernels.def"
#undef X
  kAsmCount
};

// the standard-argument kernels: one workgroup per block of the kernel's row length.  ny > 0: only the moduli [0, ny) of every
// polynomial (grid.y; rows stay nm apart) -- the delta-form prefix of a context whose later moduli take the general family
hipError_t launch_asm(AsmKind kind, const Shape &s, const DevTables &t, uint64_t *c, const uint64_t *a, const uint64_t *b,
                      size_t batch, hipStream_t st, int ny = 0);
// ... the stand-alone transforms that take two polynomials (same modulus) per workgroup; batch >= 2
hipError_t launch_asm_x2(AsmKind kind, const Shape &s, const DevTables &t, uint64_t *dst, const uint64_t *src, size_t batch,
                         hipStream_t st, int ny = 0);
hipError_t warm_asm(hipStream_t st);   // first use: loads the generated kernels' module and this unit's own code object

}  // namespace nflhip
