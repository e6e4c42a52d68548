// healpix_geom.h - the one HEALPix geometry of the library, shared by pmesh.hip, hpinterp.hip, pointsource.hip and
// galaxy.hip: the RING pixel-centre arithmetic of cora_amd/util/hputil.py (pix2ang, ang2pix), repeated operation for
// operation so that the host oracles and the kernels pick the same pixels (no contraction into FMAs there), and the
// NESTED hierarchy: RING pixel <-> (x, y, face) at any nside, RING <-> NESTED index at a power of two, the child offsets
// and the balanced-tree sum over NESTED children.  Restated from the published HEALPix algorithm (Gorski et al. 2005).
#pragma once
#include "common.h"

#include <cmath>

namespace {

struct Geom {
    long nside, npix, ncap;
};

inline Geom make_geom(int nside) {
    Geom g;
    g.nside = nside;
    g.npix = 12L * nside * nside;
    g.ncap = 2L * nside * (nside - 1);
    return g;
}

__device__ inline long isqrt_l(long v) {
    long r = (long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

__device__ inline long floordiv_l(long a, long b) {
    long q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}
__device__ inline long floormod_l(long a, long b) { return a - floordiv_l(a, b) * b; }

// numpy's float remainder (npy_divmod): fmod, moved to the sign of the divisor
__device__ inline double np_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// z and phi of a pixel centre: the arithmetic of hputil.pix2ang, in the same order
__device__ inline void pix2zphi(const Geom &g, long ipix, double &z, double &phi) {
#pragma clang fp contract(off)
    const long ns = g.nside;
    const double dn = (double)ns;
    if (ipix < g.ncap || ipix >= g.npix - g.ncap) {
        const bool south = ipix >= g.ncap;
        long p = south ? g.npix - 1 - ipix : ipix;
        long i = (1 + isqrt_l(1 + 2 * p)) >> 1;     // ring (1-based) holding 2 i (i - 1) .. 2 i (i + 1) - 1
        long j = p - 2 * i * (i - 1);
        double zc = 1.0 - (double)i * (double)i / (3.0 * dn * dn);
        double pc = ((double)j + 0.5) * M_PI / (2.0 * (double)i);
        z = south ? -zc : zc;
        phi = south ? 2.0 * M_PI - pc : pc;
    } else {
        long pb = ipix - g.ncap;
        long i = pb / (4 * ns) + ns;
        long j = pb % (4 * ns);
        long s = (i - ns + 1) & 1;
        z = 4.0 / 3.0 - 2.0 * (double)i / (3.0 * dn);
        phi = ((double)j + 0.5 * (double)s) * M_PI / (2.0 * dn);
    }
}

// healpy.pix2vec: (sin theta cos phi, sin theta sin phi, z) with sin theta = sqrt((1 - z)(1 + z))
__device__ inline void pix2vec(const Geom &g, long ipix, double v[3]) {
#pragma clang fp contract(off)
    double z, phi;
    pix2zphi(g, ipix, z, phi);
    double st = sqrt((1.0 - z) * (1.0 + z));
    double s, c;
    sincos(phi, &s, &c);
    v[0] = st * c;
    v[1] = st * s;
    v[2] = z;
}

// RING ang2pix: the arithmetic of hputil.ang2pix, in the same order
__device__ inline long ang2pix(const Geom &g, double theta, double phi) {
#pragma clang fp contract(off)
    const long ns = g.nside;
    const double dn = (double)ns;
    double z = cos(theta);
    double za = fabs(z);
    double tt = np_mod(phi, 2.0 * M_PI) / (M_PI / 2.0);
    if (za <= 2.0 / 3.0) {
        double t1 = dn * (0.5 + tt);
        double t2 = dn * z * 0.75;
        long jp = (long)floor(t1 - t2);
        long jm = (long)floor(t1 + t2);
        long ir = ns + 1 + jp - jm;
        long kshift = 1 - (ir & 1);
        long ip = floormod_l(floordiv_l(jp + jm - ns + kshift + 1, 2), 4 * ns);
        return g.ncap + (ir - 1) * 4 * ns + ip;
    }
    double tp = tt - floor(tt);
    double tmp = dn * sqrt(3.0 * (1.0 - za));
    long jp = (long)floor(tp * tmp);
    long jm = (long)floor((1.0 - tp) * tmp);
    long irc = jp + jm + 1;
    long ipc = floormod_l((long)floor(tt * (double)irc), 4 * irc);
    return z > 0 ? 2 * irc * (irc - 1) + ipc : g.npix - 2 * irc * (irc + 1) + ipc;
}

// pmesh.calculate_positions for one particle: theta outside [0, pi] is reflected and phi gains pi, then phi mod 2 pi
__device__ inline void displaced_position(double thp, double php, double dth, double dph, double &th, double &ph) {
#pragma clang fp contract(off)
    th = thp + dth;
    ph = php + dph;
    if (th > M_PI || th < 0.0) {
        th = M_PI - np_mod(th, M_PI);
        ph = ph + M_PI;
    }
    ph = np_mod(ph, 2.0 * M_PI);
}

// ---- NESTED hierarchy --------------------------------------------------------------------------------------------

// the southern corner of base face f: its ring in units of nside, {2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4}, and its longitude
// in units of pi / 4, {1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7}.  Computed, not tabulated: no memory access in the lane.
__device__ inline int face_jrll(int f) { return (f >> 2) + 2; }
__device__ inline int face_jpll(int f) { return 2 * (f & 3) + ((f >> 2) == 1 ? 0 : 1); }

// RING pixel -> (x, y, face): x runs to the north-east, y to the north-west, inside base pixel `face`.  I: the type the
// caller keeps its coordinates in (int or long; they are below nside); the arithmetic is 64-bit for either.
template <typename I>
__device__ inline void ring2xyf(const Geom &g, long pixel, I &ix, I &iy, int &face) {
    const long ns = g.nside, nl2 = 2 * ns;
    long iring, iphi, kshift, nr;
    if (pixel < g.ncap) {
        iring = (1 + isqrt_l(1 + 2 * pixel)) >> 1;
        iphi = pixel + 1 - 2 * iring * (iring - 1);
        kshift = 0;
        nr = iring;
        face = (int)((iphi - 1) / nr);
    } else if (pixel < g.npix - g.ncap) {
        const long ip = pixel - g.ncap;
        const long tmp = ip / (4 * ns);
        iring = tmp + ns;
        iphi = ip - tmp * 4 * ns + 1;
        kshift = (iring + ns) & 1;
        nr = ns;
        const long ire = tmp + 1, irm = nl2 + 1 - tmp;
        const long ifm = (iphi - (ire >> 1) + ns - 1) / ns, ifp = (iphi - (irm >> 1) + ns - 1) / ns;
        face = (int)(ifp == ifm ? (ifp | 4) : (ifp < ifm ? ifp : ifm + 8));
    } else {
        const long ip = g.npix - pixel;
        iring = (1 + isqrt_l(2 * ip - 1)) >> 1;
        iphi = 4 * iring + 1 - (ip - 2 * iring * (iring - 1));
        kshift = 0;
        nr = iring;
        iring = 2 * nl2 - iring;
        face = 8 + (int)((iphi - 1) / nr);
    }
    const long irt = iring - face_jrll(face) * ns + 1;
    long ipt = 2 * iphi - face_jpll(face) * nr - kshift - 1;
    if (ipt >= nl2) ipt -= 8 * ns;
    ix = (I)((ipt - irt) >> 1);
    iy = (I)((-ipt - irt) >> 1);
}

template <typename I>
__device__ inline long xyf2ring(const Geom &g, I ix, I iy, int face) {
    const long ns = g.nside, nl4 = 4 * ns;
    const long jr = face_jrll(face) * ns - ix - iy - 1;
    long nr, kshift, before;
    if (jr < ns) {
        nr = jr;
        before = 2 * nr * (nr - 1);
        kshift = 0;
    } else if (jr > 3 * ns) {
        nr = nl4 - jr;
        before = g.npix - 2 * (nr + 1) * nr;
        kshift = 0;
    } else {
        nr = ns;
        before = g.ncap + (jr - ns) * nl4;
        kshift = (jr - ns) & 1;
    }
    long jp = (face_jpll(face) * nr + ix - iy + 1 + kshift) / 2;
    if (jp > nl4) jp -= nl4;
    else if (jp < 1) jp += nl4;
    return before + jp - 1;
}

// every second bit of j, from bit `from`: the x (from = 0) or y (from = 1) offset of NESTED child j
__device__ inline long child_offset(long j, int from, int k) {
    long v = 0;
    for (int b = 0; b < k; b++) v |= ((j >> (2 * b + from)) & 1L) << b;
    return v;
}

// the bits of v spread onto the even places
__device__ inline long spread_bits(long v, int k) {
    long r = 0;
    for (int b = 0; b < k; b++) r |= ((v >> b) & 1L) << (2 * b);
    return r;
}

// RING <-> NESTED pixel at nside = 2^k: NESTED pixel q = face nside^2 + (x bits on the even places, y bits on the odd)
__device__ inline long nest2ring_dev(const Geom &g, int k, long q) {
    const long nn = g.nside * g.nside;
    const int face = (int)(q / nn);
    const long j = q - face * nn;
    return xyf2ring(g, child_offset(j, 0, k), child_offset(j, 1, k), face);
}

__device__ inline long ring2nest_dev(const Geom &g, int k, long p) {
    long ix, iy;
    int face;
    ring2xyf(g, p, ix, iy, face);
    return (long)face * g.nside * g.nside + (spread_bits(ix, k) | (spread_bits(iy, k) << 1));
}

// RING pixel at gin (nside 2^k times finer) of NESTED child j of the pixel (ix, iy, face)
__device__ inline long child_pixel(const Geom &gin, long ix, long iy, int face, int k, long j) {
    return xyf2ring(gin, (ix << k) + child_offset(j, 0, k), (iy << k) + child_offset(j, 1, k), face);
}

// One step of the balanced-tree sum over j = 0, 1, 2, ...: v joins the partial sums of the set low bits of j (a binary
// counter), so that after j = 2^n - 1 part[n] holds the pairwise sum of all 2^n values, in which equal values sum
// exactly.  Every user sums through this one function: the same operations in the same order.
__device__ inline void tree_push(double *part, long j, double v) {
    int lvl = 0;
    for (; (j >> lvl) & 1; lvl++) v = part[lvl] + v;
    part[lvl] = v;
}

__global__ __launch_bounds__(256) void minus_one_kernel(double *__restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] -= 1.0;
}

}  // namespace
