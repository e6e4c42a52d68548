// glibc_exp.h - glibc's exp restated for the device, shared by npnormal.hip (ziggurat wedge test) and lsschain.hip
// (lognormal transform).
#pragma once
#include <hip/hip_runtime.h>

// glibc's exp (sysdeps/ieee754/dbl-64/e_exp.c: x = k ln2 / 128 + r, 2^(k/128) from a 128-entry table of (tail, scale
// bits), exp(r) - 1 by a degree-5 polynomial) in the evaluation order of its FMA build - the one the loader selects on
// every CPU with FMA + AVX2, read off the installed libm's code - operation by operation: what is fused there is an fma
// here, what is separate stays separate (contraction off).  Constants: glibc_exp_tab.inc (tools/gen_glibc_exp_tab.py
// reads them out of the installed libm).  For |x| < 512 (the wedge test's argument is in [-6.7, 0)); oracle/npnormal.py
// restates the same sequence and tests/test_oracle.py pins it to the host's exp bit for bit.
#include "glibc_exp_tab.inc"
static __device__ const ulonglong2 g_gexp_T[128] = GLIBC_EXP_T;
__device__ inline double glibc_exp_fma(double x) {
#pragma clang fp contract(off)
    constexpr double C[4] = GLIBC_EXP_C;
    const unsigned abstop = ((unsigned)__double2hiint(x) >> 20) & 0x7ffu;
    if (abstop < 0x3c9u) return 1.0 + x;                          // |x| < 2^-54
    double kd = fma(x, GLIBC_EXP_INVLN2N, GLIBC_EXP_SHIFT);
    const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
    kd = kd - GLIBC_EXP_SHIFT;
    const double r = fma(kd, GLIBC_EXP_NEGLN2LON, fma(kd, GLIBC_EXP_NEGLN2HIN, x));
    const ulonglong2 t = g_gexp_T[ki & 127ull];
    const double tail = __longlong_as_double((long long)t.x);
    const unsigned long long sbits = t.y + (ki << 45);
    const double p23 = fma(r, C[1], C[0]);
    const double tr = r + tail;
    const double r2 = r * r;
    const double p45 = fma(r, C[3], C[2]);
    const double t1 = fma(p23, r2, tr);
    const double r4 = r2 * r2;
    const double tmp = fma(r4, p45, t1);
    const double scale = __longlong_as_double((long long)sbits);
    return fma(scale, tmp, scale);
}
