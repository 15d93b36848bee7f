// Wrapper that lets hipcc read the reference's cudabits/arraylet2.cu (+ common.h) as HIP source, unchanged, found on the
// include path at build time (oracle/ref_kernels.py).  This file is the project's own text; nothing of the reference is copied.
#include <hip/hip_runtime.h>
// common.h:4 defines atomicAdd(double*, double), which HIP already has: give the reference's (unused) copy another name
#define atomicAdd ref_atomicAdd
// arraylet2.cu:28-41 holds an unused double shuffle whose two moves are PTX inline assembly: drop the two statements
#define asm
#define volatile(...)
#include "cudabits/arraylet2.cu"
