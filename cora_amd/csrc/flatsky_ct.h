// flatsky_ct.h - what flatsky.hip calls in flatsky_ct.hip: the flat-sky line transforms on the compile-time FFT passes.
// Every pass function returns the error status only (0 = OK) and sets *took: true if the pass was launched here, false
// if flatsky.hip's generic line kernel has to take it ("launched" cannot share the status int: see sht_ringfft_ct).
#pragma once
#include "common.h"

// plan time: the compile-time convolution length for an n-point Bluestein line and its filter; *Pct = 0: none
int flat_blu_plan(corahip_ctx *ctx, int n, const double2 *chirp, int *Pct, dev_buf<double2> *filt_ct);
// contiguous passes of an even real length 2 h
int flat_c2r_ct(corahip_ctx *ctx, const double *spec, double *out, long nlines, int h, double scale, bool *took);
int flat_r2c_ct(corahip_ctx *ctx, const double *in, double *spec, long nlines, int h, bool *took);
int flat_blu_real_ct(corahip_ctx *ctx, bool c2r, const double *in, double *out, long nlines, int h, double scale, int Pct,
                     const double2 *chirp, const double2 *filt_ct, const double2 *rtw, bool *took);
// strided complex passes (inner > 1); gen: the input is generated from the real k-weights `in`
int flat_c2c_ct(corahip_ctx *ctx, const double *in, double *out, long nouter, int n, long inner, int inverse, double scale, bool gen,
                uint64_t seed, bool *took);
int flat_blu_c2c_ct(corahip_ctx *ctx, const double *in, double *out, long nouter, int n, long inner, int inverse, double scale, bool gen,
                    uint64_t seed, int Pct, const double2 *chirp, const double2 *filt_ct, bool *took);
