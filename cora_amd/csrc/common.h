// common.h - internals shared by the translation units of libcorahip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/corahip.h"
#include "dev_buf.h"

void corahip_set_error(const char *fmt, ...);

struct corahip_prof_entry {
    double total_ms = 0.0;
    int launches = 0;
};

struct corahip_pending_event {
    std::string name;
    hipEvent_t e0, e1;
};

// tables of one line-FFT length of the flat-sky engine (flatsky.hip); device buffers
struct corahip_linefft_plan {
    int n = 0, P = 0, logP = 0, blu = 0;
    int Pct = 0;               // Bluestein lengths: convolution length of the compile-time passes (flatsky_ct.hip), 0 = none
    dev_buf<double2> filt_ct;     // [Pct] its filter, in the passes' storage order
    dev_buf<double2> tw;       // [P]  exp(-2 pi i k / P)
    dev_buf<double2> chirp;    // [n]  exp(-i pi k^2 / n)                       (Bluestein lengths only)
    dev_buf<double2> filt;     // [P]  FFT_P(wrapped conj chirp) / P, bit-reversed (Bluestein lengths only)
    dev_buf<double2> rtw;      // [n/2 + 1]  e^{+2 pi i k / 2n}: (un)packing of a real transform of length 2n
};

#define CORAHIP_NSCRATCH 13
struct corahip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;                 // second stream for kernels that run beside those of `stream` (K5 pair)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    dev_buf<int> k5_tickets;                       // K5: the item counters of the ticketed belt kernel (8 words, zeroed per call)
    // the l-range pipeline of the numpy-stream draw (drawstream.hip): its generator stream and the ring's events
    dev_buf<unsigned> draw_slot_tab[2];            // K3: (l, m block) of every work slot of 0 .. draw_slot_lmax, for blocks of
    int draw_slot_lmax[2] = {-1, -1};              //     128 m ([0]) and of 64 m ([1], the wide shape) (draw.hip)
    bool mt_plist_ready = false;                   // scratch slot 9 holds the position lists (mtlegacy.hip)
    hipStream_t gen_stream = nullptr;
    hipEvent_t ev_ring[8] = {};
    // the session of corahip_draw_alm_numpy_prepare that has not seen its _end yet (_end alone frees a session): its
    // generator tables (scratch slot 6) and ring (slot 7) are in use by queued launches, so a second _prepare and the
    // whole-stream generators (corahip_normals_pcg64 / _mt19937_legacy, which share slot 6) return CORAHIP_ESTATE until then
    const void *draw_pending = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool profile = false;
    std::map<std::string, corahip_prof_entry> prof;
    std::vector<corahip_pending_event> pending;
    int num_cu = 256;
    size_t total_mem = 0;                          // device memory (bytes)
    // grow-only device scratch slots owned by the context
    // slots: 0 K1 transposed tables, 1 K1 pair results / odd-F normal stream, 2 K1 pair list, 3 zeros,
    //        4 Legendre matrix of legendre_project, 5 its zero-padded operand, 6 block tables of normals_pcg64 /
    //        segment tables of normals_mt19937_legacy, 7 the two-slot ring of the l-range pipeline (drawstream.hip),
    //        8 barrier words of the cooperative Cholesky, 9 position lists of the MT19937 jump polynomials,
    //        10 block partials of complex_variance (faraday.hip) and of field_moments with its column sums (lofar.hip), 11 per-pixel source offsets of pointsource_paint,
    //        12 spline records + interval lookup table of xi_multi_average (corrfunc.hip)
    //  written whole by every call that reads them: 1, 3, 4, 5, 6, 7, 8, 10, 11, 12; caches behind a host flag: 0
    //  (tt_valid), 2 (pairs_key / pairs_ptr), 9 (mt_plist_ready)
    dev_buf<char> scratch[CORAHIP_NSCRATCH];
    size_t scratch_bytes[CORAHIP_NSCRATCH] = {};
    // corahip_debug_poison_scratch (tests): the byte every newly allocated scratch slot and per-call device allocation
    // is filled with, -1 = none (the default)
    int debug_poison = -1;
    // K1 transposed tables resident in scratch slot 0: valid for the pinned (dd, dv, vv, generation) only
    // (corahip_clarray_tables_pin: the caller vouches that the tables do not change under that generation)
    const void *tt_pin[3] = {nullptr, nullptr, nullptr};
    uint64_t tt_pin_gen = 0;
    bool tt_pinned = false, tt_valid = false;
    hipStream_t tt_stream = nullptr;               // stream the kept copy was made on
    // K1 pair list resident in scratch slot 2: (F, first, step, slots, device pointer it was written to)
    long pairs_key[4] = {-1, -1, -1, -1};
    void *pairs_ptr = nullptr;
    // flat-sky line-FFT tables by transform length
    std::map<int, corahip_linefft_plan> linefft;
};

// returns a device buffer of at least `bytes` for `slot`, reallocating only when it must grow
int corahip_ctx_scratch(corahip_ctx *ctx, int slot, size_t bytes, void **out);
// fills a per-call device allocation with the poison byte of corahip_debug_poison_scratch, if one is set (tests)
int corahip_debug_fill(corahip_ctx *ctx, void *p, size_t bytes);

// RAII: HIP-event pair around the launches of one named stage when profiling is on.
struct StageTimer {
    corahip_ctx *ctx;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const char *name;
    hipStream_t stream;
    // `on`: the stream the timed launches go to (default: the context's; the events of another stream must have completed
    // by the time the context's stream is drained - true for the side streams of the library, which it always joins)
    StageTimer(corahip_ctx *c, const char *n, hipStream_t on = nullptr, bool other = false) : ctx(c), name(n), stream(other ? on : c->stream) {
        if (ctx->profile) {
            (void)hipEventCreate(&e0);
            (void)hipEventCreate(&e1);
            (void)hipEventRecord(e0, stream);
        }
    }
    ~StageTimer() {
        if (ctx->profile) {
            (void)hipEventRecord(e1, stream);
            ctx->pending.push_back({name, e0, e1});
        }
    }
};

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            corahip_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                              __FILE__, __LINE__);                                          \
            return (int)_e;                                                                 \
        }                                                                                   \
    } while (0)

#define ARG_CHECK(cond)                                                                     \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            corahip_set_error("invalid argument: %s (%s:%d)", #cond, __FILE__, __LINE__);   \
            return CORAHIP_EINVAL;                                                          \
        }                                                                                   \
    } while (0)

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

// ---- host-side launch helpers of the streaming entry points (the K1-K5 launches are tuned per kernel, not these) ----

// blocks of 256 threads for a grid-stride kernel over n elements: ceil(n / 256), at most per_cu per CU, at least 1
static inline unsigned grid_blocks(const corahip_ctx *ctx, long n, int per_cu = 16) {
    long blocks = (n + 255) / 256;
    const long cap = (long)ctx->num_cu * per_cu;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// an ordered two-pass sum over `count` elements: the number of block partials nb (at most 4096, ~8192 elements each) and
// the elements per partial, rounded up to a multiple of `round` (1 or 2) - a function of count alone
static inline void partials_split(long count, int round, int *nb, long *per) {
    long b = (count + 8191) / 8192;
    if (b > 4096) b = 4096;
    long pr = (count + b - 1) / b;
    pr = (pr + round - 1) & ~(long)(round - 1);
    *nb = (int)((count + pr - 1) / pr);
    *per = pr;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  A null pointer (an optional argument left out) overlaps
// nothing.  The guard changes no accepted call of the entry points that used to test without it: a null b "overlapped"
// only an a below nb, and a real device pointer is never smaller than a buffer length.
static inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

// log2 of a power of two, -1 for anything else
static inline int log2_exact(int v) {
    int k = 0;
    while ((1 << k) < v) k++;
    return (1 << k) == v ? k : -1;
}

// p on a multiple of `bytes` (a power of two); true for a null pointer
static inline bool is_aligned(const void *p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

__host__ __device__ static inline long nalm_of(int lmax) { return (long)(lmax + 1) * (lmax + 2) / 2; }
// healpy packed index (m-major): idx(l,m) = m(2 lmax+1-m)/2 + l
__host__ __device__ static inline long alm_idx(int l, int m, int lmax) {
    return (long)m * (2 * lmax + 1 - m) / 2 + l;
}

// l of packed index idx: m is the last one whose first entry (l = m), at m (2 lmax + 3 - m) / 2, is not beyond idx
__device__ static inline long alm_l_of_idx(long idx, int lmax) {
    const double b = 2.0 * lmax + 3.0;
    long m = (long)((b - sqrt(b * b - 8.0 * (double)idx)) * 0.5);
    m = m < 0 ? 0 : (m > lmax ? lmax : m);
    while (m > 0 && m * (2L * lmax + 3 - m) / 2 > idx) m--;
    while (m < lmax && (m + 1) * (2L * lmax + 2 - m) / 2 <= idx) m++;
    return idx - m * (2L * lmax + 1 - m) / 2;
}

typedef double d4_t __attribute__((ext_vector_type(4)));

// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>), in order
template <int N, int J = 0, class Fn>
__device__ static inline void static_for(Fn &&f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J>{});
        static_for<N, J + 1>(f);
    }
}

// sums of 256 threads' (a, b) in a fixed order, returned to every thread: lanes by halving __shfl_down from 32 to 1,
// then ((w0 + w1) + w2) + w3 over the four waves through red[8] (LDS)
__device__ static inline void block_sum2(double &a, double &b, double *red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[2 * wave] = a, red[2 * wave + 1] = b;
    __syncthreads();
    a = ((red[0] + red[2]) + red[4]) + red[6];
    b = ((red[1] + red[3]) + red[5]) + red[7];
}

// op over the values of the NT threads of a workgroup (NT a power of two) by a halving tree in red [NT] (LDS):
// red[t] = op(red[t], red[t + s]) for s = NT / 2 .. 1, a fixed order; the result goes to every thread.  Ends with a
// barrier, so red may be reused at once; whatever the threads wrote before the call is published by it as well.
template <int NT, class Op>
__device__ __forceinline__ double block_reduce(double v, double *red, Op op) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = op(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
