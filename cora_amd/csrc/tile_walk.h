// tile_walk.h - how the persistent workgroups of the flat-sky line kernels (flatsky.hip, flatsky_ct.hip) walk the tiles
// of a STRIDED axis: element j of line (outer, i) lives at (outer n + j) inner + i, a tile is NCH lines that are
// neighbours along the contiguous axis, chunks = ceil(inner / NCH) tiles per outer index, nouter chunks tiles in all.
#pragma once

#ifndef FS_PAIR_XCD
#define FS_PAIR_XCD 3   // log2 of the adjacent tiles given to one XCD at a time (0: off); measured 1024^3 axis-1 pass: 7.05 / 6.44 / 6.2 / 6.08 ms for 0 / 1 / 2 / 3
#endif

struct tile_t {
    long base;   // offset of element 0 of the tile's first line
    int teff;    // lines of the tile that exist (the last chunk of an outer index may be short)
};

// NCH: lines per tile (0: given at run time), N: elements per line where that is a compile-time value (0: passed to
// tile_of), GL: log2 of the tiles per group.
// Strided axes read and write 16 NCH-byte segments: two tiles that are neighbours along the contiguous axis share every
// 128-byte line (the row pitch is odd in 16-byte units).  Workgroups b and b + 8 run on the same XCD (round-robin
// dispatch) at the same time, so they (and b + 16, ...) are given adjacent tiles, 2^GL at a time, and a line is fetched
// into that XCD's L2 once instead of into several L2s.
// Two steps, because the compiler leaves scalar code where it is written: the constructor at the top of a kernel,
// pair_xcds() behind the kernel's own preamble (the measured kernels have the test there).
template <int NCH, int N = 0, int GL = FS_PAIR_XCD>
struct tile_walk {
    long inner, chunks;
    bool pair_xcd;
    __device__ __forceinline__ tile_walk(long inner_, int nch = NCH) : inner(inner_), chunks((inner_ + nch - 1) / nch) {}
    // whole groups on both sides only: every workgroup then meets whole groups
    __device__ __forceinline__ void pair_xcds(long ntiles, bool allowed = true) {
        const long gmask = (8L << GL) - 1;
        pair_xcd = GL > 0 && allowed && (ntiles & gmask) == 0 && (gridDim.x & gmask) == 0;
    }
    // v-th tile in launch order (v = blockIdx.x + k gridDim.x) -> tile index
    __device__ __forceinline__ long remap(long v) const {
        if (!pair_xcd) return v;
        const long slot = v >> 3, xcd = v & 7;
        return (((slot >> GL) * 8 + xcd) << GL) + (slot & ((1 << GL) - 1));
    }
    // the v-th tile of lines of n elements
    __device__ __forceinline__ tile_t tile_of(long v, int n = N) const {
        static_assert(NCH > 0, "compile-time tile shape");
        const long tile = remap(v);
        const long outer = tile / chunks, i0 = (tile - outer * chunks) * NCH;
        tile_t t;
        t.base = outer * (N ? N : n) * inner + i0;
        t.teff = (int)min((long)NCH, inner - i0);
        return t;
    }
};
