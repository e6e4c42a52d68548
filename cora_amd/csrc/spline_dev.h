// spline_dev.h - one evaluation of a natural cubic spline with end-slope extrapolation (cubicspline.pyx:126-175) on
// values, and the bisection that fills a look-up cell: shared by corrfunc.hip (xi_table_kernel from LDS, xi_multi_kernel
// from interval records) and rsdcorr.hip (xi_rsd_kernel from interval records).
#pragma once

__device__ static inline double spline_below(double x0, double x1, double y0, double y1, double z1, double x) {
    const double h = x1 - x0;
    return ((y1 - y0) / h - h * z1 / 6.0) * (x - x0) + y0;
}
__device__ static inline double spline_above(double xm, double xn, double ym, double yn, double zm, double x) {
    const double h = xn - xm;
    return ((yn - ym) / h + h * zm / 6.0) * (x - xn) + yn;
}
__device__ static inline double spline_interp(double xk, double xk1, double ih, double h2o6, double yk, double yk1,
                                              double zk, double zk1, double x) {
    const double a = (xk1 - x) * ih, b = (x - xk) * ih;
    return a * yk + b * yk1 + ((a * a * a - a) * zk + (b * b * b - b) * zk1) * h2o6;
}
// lut[g]: bisection for the last knot at or before the left edge of cell g
__device__ static inline int spline_lut_cell(const double *xs, int nk, double xl) {
    int kl = 0, kh = nk;
    while (kh - kl > 1) {
        const int kn = (kh + kl) >> 1;
        if (xs[kn] > xl) kh = kn;
        else kl = kn;
    }
    return kl;
}
