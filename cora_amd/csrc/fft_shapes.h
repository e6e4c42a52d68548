// fft_shapes.h - the compile-time transform shapes of the two FFT engines, stated once: which lengths have a kernel with
// a fixed schedule (fft_ct.h, Sch<len>), with how many channels / lines per item and how many threads.  Host-side data
// only.  The dispatchers of sht_ringfft_ct.hip and flatsky_ct.hip instantiate one kernel per row through dispatch();
// the plan (sht_plan.hip), the scheduler's weights and the filter builders read the same rows at run time.  Adding or
// retuning a length is one row here (and its Sch<> in fft_ct.h).
#pragma once
#include <cstddef>
#include <type_traits>
#include <utility>

namespace fft_shapes {

// ---- ring transforms (K5 synthesis / K5^T analysis) ----------------------------------------------------------------
struct ring_shape {
    int len;        // transform length: h of the belt rings (direct), Bluestein convolution length (cap rings)
    int nch;        // channels per item (and per workgroup)
    int mc;         // synthesis: cells prefetched per thread and channel group
    int t;          // synthesis: threads per workgroup
    int ana_t;      // analysis: threads per workgroup, 0 = the run-time ringana_kernel takes the class
    bool own;       // Bluestein: the filters come from the plan's second set, stored in the order of the compile-time
                    // passes (false: a power of two whose filter in the plan's first set has that order anyway)
    double us;      // CU microseconds per item, the CU not limited by HBM (measurement: sht_ringfft_item_weight)
};
// the belt; both rows draw their items from the context's tickets.  The analysis kernel is taken only when lmax <= len.
inline constexpr ring_shape RING_DIRECT[] = {
    {2048, 4, 4, 512, 512, false, 9.9},
    {4096, 2, 8, 512, 512, false, 12.7},
};
// 8192 / 6144: one channel fills the LDS.  Measured at the cfg-5 rank share (128 channels; the generic kernel took
// 30.6 ms for the two classes): 512 threads (two waves per SIMD, but the radix-32 / 24 butterflies then spill: 268 / 72
// bytes) 16.5 / 10.1 ms, 256 threads (one wave per SIMD, no spill) 13.8 / 10.8 ms for 8192 / 6144: each takes the
// faster form.  1024: 256 threads, two workgroups per CU: 0.61 -> 0.54 ms.
inline constexpr ring_shape RING_BLU[] = {
    {8192, 1, 16, 256, 0, true, 26.1},
    {6144, 1, 8, 512, 0, true, 20.5},
    {4096, 2, 4, 512, 512, false, 15.0},
    {3584, 2, 4, 512, 512, true, 14.3},
    {3072, 2, 4, 512, 512, true, 13.3},
    {2560, 2, 4, 512, 512, true, 12.4},
    {2048, 4, 2, 512, 512, false, 12.6},
    {1536, 4, 2, 512, 512, true, 10.6},
    {1024, 4, 2, 256, 256, false, 6.8},
};
constexpr bool has_analysis(const ring_shape &s) { return s.ana_t != 0; }
constexpr bool own_filter(const ring_shape &s) { return s.own; }

// ---- flat-sky lines ------------------------------------------------------------------------------------------------
struct line_shape {
    int len;                // complex transform length (real passes: h of the real length 2 h)
    int nch;                // lines per item
    int t = 512;            // threads per workgroup
    int t_c2r = 512;        // real passes: threads of the half-complex -> real kernel (t: real -> half-complex)
    bool h2 = false;        // strided c2c: the half-tile kernel, one workgroup per CU (linec2c_h2_ct)
    int inner_min = 0;      // strided c2c: smallest inner extent the row takes
};
// contiguous real passes (liner2c_ct / linec2r_ct)
inline constexpr line_shape LINE_REAL[] = {
    {256, 16, 512, 256}, {512, 16}, {1024, 8}, {2048, 4}, {192, 16, 512, 256}, {384, 16}, {768, 8}, {1536, 4},
};
// strided complex passes (linec2c_ct / linec2c_h2_ct): the first row that matches length and inner extent wins
inline constexpr line_shape LINE_C2C[] = {
    {256, 16, 256, 256, false, 16}, {512, 16, 512, 512, false, 16}, {1024, 16, 512, 512, true, 16},
    {1024, 8, 512, 512, false, 8},  {384, 16, 512, 512, false, 16}, {768, 8, 512, 512, false, 8},
};
// Bluestein convolution lengths, ascending: a line of n points takes the first that holds 2 n - 1
inline constexpr line_shape LINE_BLU[] = {
    {256, 16},  {320, 16},  {384, 16},  {512, 16},  {640, 8},  {768, 8},  {1024, 8},
    {1280, 4},  {1536, 4},  {2048, 4},  {2560, 2},  {3072, 2}, {3584, 2}, {4096, 2},
};
constexpr int LINE_BLU_FILTER_T = 256;   // threads of the plan-time filter kernel (flat_blu_filter_kernel)

// what the kernels assert per instantiation, here per table: every thread loads whole butterflies / whole lines
template <size_t N>
constexpr bool whole_loads(const line_shape (&rows)[N]) {
    for (const line_shape &s : rows)
        if ((s.nch * s.len) % s.t != 0 || (s.nch * s.len) % s.t_c2r != 0) return false;
    return true;
}
static_assert(whole_loads(LINE_REAL) && whole_loads(LINE_C2C) && whole_loads(LINE_BLU), "(NCH * N) % T == 0");

// ---- run-time readers ----------------------------------------------------------------------------------------------
template <class S, size_t N>
constexpr const S *find(const S (&rows)[N], int len) {
    for (const S &s : rows)
        if (s.len == len) return &s;
    return nullptr;
}
// the length with a filter set of its own that the compile-time kernels take for a cap ring of half length h whose
// generic (power-of-two) Bluestein length is P: the shortest such length in [2 h - 1, P]; 0 = none
constexpr int ring_own_length(int h, int P) {
    int best = 0;
    for (const ring_shape &s : RING_BLU)
        if (s.own && s.len >= 2 * h - 1 && s.len <= P && (best == 0 || s.len < best)) best = s.len;
    return best;
}

// ---- dispatch --------------------------------------------------------------------------------------------------------
// A row as a type: `shape.row` is a constant expression inside a generic lambda, so its fields can be template arguments.
template <const auto &ROWS, size_t I>
struct row_c {
    static constexpr auto row = ROWS[I];
};
template <auto KEEP, class S>
constexpr bool kept(const S &s) {
    if constexpr (std::is_null_pointer_v<decltype(KEEP)>) return true;
    else return KEEP(s);
}
template <const auto &ROWS, auto KEEP, size_t... I, class Match, class Launch>
int dispatch_rows(std::index_sequence<I...>, Match match, Launch launch, bool *took) {
    int rc = 0;
    auto one = [&](auto shape) {
        if constexpr (kept<KEEP>(shape.row)) {
            if (!match(shape.row)) return false;
            rc = launch(shape);
            *took = rc == 0;
            return true;
        } else {
            return false;
        }
    };
    (void)(one(row_c<ROWS, I>{}) || ...);
    return rc;
}
// Calls launch(shape) for the first row of ROWS that KEEP (compile time, a constexpr function of the row or nullptr for
// every row: rows it rejects instantiate nothing) and match (run time) accept.  The return value is the error status of
// the launch only (0 = OK, or where no row matched); *took = a kernel was launched.  hipErrorInvalidValue is 1, so
// "launched" never shares the int with the status.
template <const auto &ROWS, auto KEEP = nullptr, class Match, class Launch>
int dispatch(Match match, Launch launch, bool *took) {
    *took = false;
    return dispatch_rows<ROWS, KEEP>(std::make_index_sequence<sizeof(ROWS) / sizeof(ROWS[0])>{}, match, launch, took);
}

// every row has a schedule: SCH<len> is defined (a missing one does not compile)
template <template <int> class SCH, const auto &ROWS, size_t... I>
constexpr bool scheduled(std::index_sequence<I...>) {
    return ((SCH<ROWS[I].len>::R0 * SCH<ROWS[I].len>::R1 * SCH<ROWS[I].len>::R2 == ROWS[I].len) && ...);
}
template <template <int> class SCH, const auto &ROWS>
constexpr bool scheduled() {
    return scheduled<SCH, ROWS>(std::make_index_sequence<sizeof(ROWS) / sizeof(ROWS[0])>{});
}

}  // namespace fft_shapes
