// sphbessel_lane.h - one lane of sphbessel_radial_kernel (fullsky.hip): the column A[0 .. lmax, i, n] of the radial table
// for one wavenumber and the NS sub-samples of one channel.  Plain C++ apart from the function qualifiers, so that a host
// program can run the same statements (the scheme is described at the top of fullsky.hip).
#pragma once
#include <cmath>
#include <cstddef>
#ifdef __HIPCC__
#define SB_HD __host__ __device__
#else
#define SB_HD
#endif

constexpr int SB_MAXSUB = 17;
constexpr int SB_TINY_LMAX = 8;               // t_{l-2} = 0 for x < 2^-170 beyond this order
constexpr double SB_TINY = 0x1p-170;
constexpr double SB_BIG = 0x1p256, SB_SMALL = 0x1p-256;

static inline int sb_lstart(int lmax) {
    const double top = (double)lmax + 1.0;
    return lmax + 1 + (int)ceil(sqrt(160.0 * top)) + 30;
}

// the contribution of one sub-sample with x < 2^-170 to order l <= SB_TINY_LMAX
SB_HD static inline double sb_tiny_term(int l, double x, double cb, double cf) {
    double t = 1.0, t2 = 0.0;                 // t_l and t_{l-2}
    for (int q = 1; q <= l; q++) {
        if (q == l - 1) t2 = t;               // (t is t_{q-1} = t_{l-2} here)
        t = t * x / (double)(2 * q + 1);
    }
    double jpp;
    if (l == 0)
        jpp = -1.0 / 3.0;
    else if (l == 1)
        jpp = -0.6 * t;
    else
        jpp = (double)(l * (l - 1)) / (double)((2 * l - 1) * (2 * l + 1)) * t2;
    return cb * t - cf * jpp;
}

// out[l * sl], l = 0 .. lmax, for the wavenumber kn; chi_i, cb_i, cf_i [nsub], nsub <= NS
template <int NS>
SB_HD static inline void sb_lane(double kn, const double *chi_i, const double *cb_i, const double *cf_i, int nsub, int lmax,
                                 int lstart, double *out, size_t sl) {
    const int top = lmax + 1;

    double v0[NS], v1[NS], ix[NS], b[NS], f[NS], fac[NS], sc[NS];
    int m[NS], r[NS];
    int L0 = top;
    unsigned tiny = 0;
#pragma unroll
    for (int a = 0; a < NS; a++) {
        const bool live = a < nsub;
        const double x = live ? kn * chi_i[a] : 0.0;
        b[a] = live ? cb_i[a] : 0.0;
        f[a] = live ? cf_i[a] : 0.0;
        fac[a] = 1.0, sc[a] = 0.0, r[a] = 0;
        if (!(x >= SB_TINY)) {
            if (live) tiny |= 1u << a;
            v0[a] = v1[a] = ix[a] = 0.0;      // contributes zeros to the general sums
            b[a] = f[a] = 0.0;
            m[a] = top;
        } else {
            double s, c;
            sincos(x, &s, &c);
            ix[a] = 1.0 / x;
            v0[a] = s * ix[a];
            v1[a] = (v0[a] - c) * ix[a];
            m[a] = x < 1.0 ? -1 : (x >= (double)top ? top : (int)x);
            L0 = m[a] < L0 ? m[a] : L0;
        }
    }

    auto tiny_sum = [&](int l) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < NS; a++)
            if (tiny >> a & 1) t += sb_tiny_term(l, kn * chi_i[a], cb_i[a], cf_i[a]);
        return t;
    };

    // ---- upward: l = 0 .. min(L0, lmax), every sub-sample at or below its turning point
    const int lasc = L0 < lmax ? L0 : lmax;
    for (int l = 0; l <= lasc; l++) {
        const double c2 = (double)l * (double)(l - 1), tl = (double)(2 * l + 3);
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < NS; a++) {
            const double jl = v0[a], jl1 = v1[a];
            const double q = c2 * ix[a] * ix[a];
            const double jpp = fma(q - 1.0, jl, 2.0 * ix[a] * jl1);
            acc = fma(b[a], jl, acc);
            acc = fma(-f[a], jpp, acc);
            if (l < lasc) {                   // the step at order l + 1 <= m_a
                v1[a] = fma(tl * ix[a], jl1, -jl);
                v0[a] = jl1;
            }
        }
        if (tiny && l <= SB_TINY_LMAX) acc += tiny_sum(l);
        out[(size_t)l * sl] = acc;
    }
    if (lasc == lmax) return;

    // ---- (1) each sub-sample upward to min(m_a, lmax); the normalisation of those that turn below top
    const int l0 = lasc < 0 ? 0 : lasc;       // the order of v0 now
#pragma unroll
    for (int a = 0; a < NS; a++) {
        if (tiny >> a & 1 || a >= nsub) continue;
        const int ta = m[a] < lmax ? m[a] : lmax;
        for (int l = l0; l < ta; l++) {
            const double t = fma((double)(2 * l + 3) * ix[a], v1[a], -v0[a]);
            v0[a] = v1[a], v1[a] = t;
        }
        if (m[a] >= top) continue;            // enters pass (2) at lmax with (j_lmax, j_top)
        const int lo = m[a] < 0 ? 0 : m[a];
        double y0 = 1.0, y1 = 0.0;
        int R = 0;
        for (int l = lstart; l > lo; l--) {
            const double t = fma((double)(2 * l + 1) * ix[a], y0, -y1);
            y1 = y0, y0 = t;
            if (fabs(y0) > SB_BIG) y0 *= SB_SMALL, y1 *= SB_SMALL, R++;
        }
        const bool use0 = m[a] < 0 || fabs(v0[a]) >= fabs(v1[a]);
        sc[a] = use0 ? v0[a] / y0 : v1[a] / y1;
        r[a] = R;
        fac[a] = R > 3 ? 0.0 : ldexp(sc[a], -256 * R);
        v0[a] = 1.0, v1[a] = 0.0;             // (y_L, y_{L+1})
    }

    // ---- (2) downward from lstart to L0 + 1, accumulating
    for (int l = lstart; l > L0; l--) {
        if (l <= lmax) {
            const double c2 = (double)l * (double)(l - 1);
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < NS; a++) {
                const double jl = v0[a] * fac[a], jl1 = v1[a] * fac[a];
                const double q = (c2 * ix[a]) * jl * ix[a];
                const double jpp = fma(2.0 * ix[a], jl1, q - jl);
                acc = fma(b[a], jl, acc);
                acc = fma(-f[a], jpp, acc);
            }
            if (tiny && l <= SB_TINY_LMAX) acc += tiny_sum(l);
            out[(size_t)l * sl] = acc;
        }
        const double tl = (double)(2 * l + 1);
#pragma unroll
        for (int a = 0; a < NS; a++) {
            if (m[a] >= top && l > lmax) continue;          // holds (j_lmax, j_top) until l = lmax
            const double t = fma(tl * ix[a], v0[a], -v1[a]);
            v1[a] = v0[a], v0[a] = t;
            if (fabs(t) > SB_BIG) {
                v0[a] *= SB_SMALL, v1[a] *= SB_SMALL;
                r[a]--;
                fac[a] = r[a] > 3 ? 0.0 : ldexp(sc[a], -256 * r[a]);
            }
        }
    }
}

