/* corahip.h - C ABI of libcorahip.so: the MI355X (gfx950) implementation of cora's
 * Gaussian-sky hot path (C_l(nu,nu') integration -> per-l factor -> correlated
 * a_lm draw -> HEALPix synthesis).
 *
 * The reference (radiocosmology/cora) has NO FFI on this path: its boundary is the
 * Python call surface of cora/core/skysim.py, cora/util/nputil.py and
 * cora/util/hputil.py.  Each entry point below names the reference code it replaces
 * (file:line relative to the reference root); cora_amd/ mirrors the Python surface
 * on top of this ABI, and INTEGRATION.md shows the ctypes stub a cora maintainer
 * would add.
 *
 * Conventions
 *  - every function returns int: 0 = OK, <0 = invalid argument (CORAHIP_E*),
 *    >0 = hipError_t of the failing runtime call.  Nothing throws across the ABI.
 *  - corahip_last_error() gives a thread-local human-readable message.
 *  - all array arguments are DEVICE pointers unless the name says `host_`; they are
 *    caller-owned (the Python side allocates them as torch tensors; hosts without
 *    torch can use corahip_malloc/free/memcpy_*).  Arrays are C-contiguous,
 *    float64 unless stated.
 *  - work is enqueued on the context's stream (corahip_ctx_set_stream) and is
 *    asynchronous; corahip_ctx_sync waits for it.
 *  - one context per GPU/process; a context is not thread-safe.
 */
#ifndef CORAHIP_H
#define CORAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORAHIP_ABI_VERSION 1
#define CORAHIP_ABI_MINOR 12     /* additions since version 1: 1 = normals_pcg64, pcg64_advance, draw_alm_rows, mkfullsky, mkfullsky_workspace_bytes, abi_minor, normals_mt19937_legacy; 2 = sht_lambda_entry (test hook); 3 = draw_alm_numpy, draw_alm_numpy_begin / _end, corahip_chanset: draw_alm_philox_rows_set, draw_alm_numpy_begin_set, randomfield_irfftn; 4 = glibc_exp (test hook), draw_alm_numpy_prepare / _run; 5 = healpix_neighbours, za_density_sph; 6 = der1_alm_prep, der1_combine, radial_gradient; 7 = slice_mix, slice_diff2, slice_moments, slice_moments_workspace_bytes, bias_field, lognormal; 8 = alm_cross_spectra; 9 = healpix_interp_weights, healpix_interp_val, healpix_rotate_maps, za_density_grid; 10 = xi_table_max_knots; 11 = complex_variance, faraday_mix, faraday_pack; 12 = pointsource_population, pointsource_paint, polarise_rotate, faraday_rotate, healpix_ud_grade, and (constrained galaxy) healpix_reorder, healpix_block_variance, alm_scale_l, galaxy_combine, and (mkconstrained) eig_top_batched, eig_top_max_f, constrained_weights, alm_mix_l, and (pk2xi) sinc_romb, fftlog_phase, logconv, logconv_split, and (initial LSS) xi_multi_average, cl_blocks, and (shot noise) normal_rows_pcg64, and (K4 lane segments) sht_lambda_segment_entry (test hook), and (poisoned scratch) debug_poison_scratch (test hook), and (redshift-space correlation) jl_romb, xi_rsd, and (LOFAR synchrotron) powerlaw_los, field_moments, and (exact curved-sky C_l) sphbessel_radial, cl_gram, clarray_fullsky_workspace_bytes, clarray_fullsky, and (polarised spectra) alm_gather_channels, and (native spin-2 analysis) map2alm_spin2_workspace_bytes, map2alm_spin2 */

#define CORAHIP_EINVAL (-1)   /* bad argument / shape */
#define CORAHIP_ENOMEM (-2)   /* workspace too small / allocation refused */
#define CORAHIP_ESTATE (-3)   /* object used in the wrong state */

typedef struct corahip_ctx corahip_ctx;
typedef struct corahip_sht_plan corahip_sht_plan;

/* ---- library / context ------------------------------------------------------------ */
int corahip_abi_version(void);
int corahip_abi_minor(void);      /* entry points added since the version was cut, see CORAHIP_ABI_MINOR */
const char *corahip_last_error(void);
int corahip_device_count(int *count);
int corahip_ctx_create(int device_id, corahip_ctx **ctx);
int corahip_ctx_destroy(corahip_ctx *ctx);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream */
int corahip_ctx_set_stream(corahip_ctx *ctx, void *hip_stream);
int corahip_ctx_sync(corahip_ctx *ctx);
/* HIP-event timing of everything enqueued between begin and end on the ctx stream (bench.py) */
int corahip_timer_begin(corahip_ctx *ctx);
int corahip_timer_end(corahip_ctx *ctx, float *elapsed_ms);
/* per-kernel accumulated HIP-event timings (enable = 1 records an event pair around every
 * kernel launch of the library; names: "clarray","factor","normals","draw","legendre","ringfft") */
int corahip_profile_enable(corahip_ctx *ctx, int enable);
int corahip_profile_get(corahip_ctx *ctx, const char *name, double *total_ms, int *launches);
int corahip_profile_reset(corahip_ctx *ctx);

/* ---- plain device memory helpers (for hosts without torch) ----------------------- */
int corahip_malloc(corahip_ctx *ctx, size_t bytes, void **dptr);
int corahip_free(corahip_ctx *ctx, void *dptr);
int corahip_memcpy_h2d(corahip_ctx *ctx, void *dst, const void *host_src, size_t bytes);
int corahip_memcpy_d2h(corahip_ctx *ctx, void *host_dst, const void *src, size_t bytes);

/* ---- K1: C_l(nu,nu') integration --------------------------------------------------
 * Replaces skysim.clarray (cora/core/skysim.py:10-69) for the two model families
 * cora ships, plus the bare Romberg reduction for arbitrary host callables.         */

/* 21cm flat-sky table model: RedshiftCorrelation.angular_powerspectrum_fft evaluation
 * (cora/signal/corr.py:944-982) with bilinearmap.interp (cora/util/bilinearmap.pyx:14-59)
 * fused with the Romberg channel average of clarray (skysim.py:41-67).
 *   dd,dv,vv   [nkperp, nkpar] lookup tables (corr.py:936-940)
 *   chi,pfd,f,b [F*zint]  per sub-sample comoving distance, prefactor*D(z)/D(z_ps),
 *                         growth rate, bias (corr.py:944-951), sub-sample s of channel i
 *                         at index i*zint+s (skysim.py:47-49 ordering)
 *   w          [zint]     normalised Romberg weights (sum = 1); zint = 1, w = {1} is zromb=0
 *   log10l     [nl]       log10 of the multipoles to evaluate (l = 0 passed as 1e-10, corr.py:957)
 *   out        [nl, F, F]
 */
int corahip_clarray_table21cm(corahip_ctx *ctx, const double *dd, const double *dv, const double *vv,
                              int nkperp, int nkpar, double kperpmin, double kperpmax, double kparmax,
                              const double *chi, const double *pfd, const double *f, const double *b,
                              int F, int zint, const double *w, const double *log10l, int nl,
                              double *out);

/* Multi-GPU form of the same integration (the reference shards clarray's output over l with
 * caput.mpiarray, skysim.py:97-103; the table lookups of a channel pair are shared by all l, so here
 * the PAIRS are sharded instead and the l-shards are assembled by one all-to-all):
 *   table21cm_pairs integrates, for all nl multipoles, the channel pairs p = pair_first + k pair_step
 *   (k = 0 .. npl-1, npl = ceil(F(F+1)/2 / pair_step); p enumerates the pairs (i, j >= i) in bands of 32 diagonals, i-major inside a band) and writes
 *   out_pairs [ceil(nl / l_block)][npl][l_block]: slab q is what the rank owning l in [q l_block, (q+1) l_block)
 *   receives.  pairs_finish takes the received slabs [nranks][npl][l_stride] (slab r from rank r) and
 *   scatters them into out [nl, F, F] and its mirror.                                              */
int corahip_clarray_table21cm_pairs(corahip_ctx *ctx, const double *dd, const double *dv, const double *vv,
                                    int nkperp, int nkpar, double kperpmin, double kperpmax, double kparmax,
                                    const double *chi, const double *pfd, const double *f, const double *b,
                                    int F, int zint, const double *w, const double *log10l, int nl,
                                    int pair_first, int pair_step, int l_block, double *out_pairs);
int corahip_clarray_pairs_finish(corahip_ctx *ctx, const double *pairs_in, int F, int nranks, int l_stride,
                                 int nl, double *out);

/* The table integrators work from an x-contiguous copy of (dd, dv, vv) that they make on every call (0.15 ms at
 * 500 x 32768).  A caller that keeps the tables unchanged between calls - they are the per-model cache of the reference,
 * cora/signal/corr.py:909-942 - pins them: the copy made by the next call is then reused as long as the SAME pointers
 * are passed and no other pin is made.  `generation` distinguishes table sets that happen to reuse device addresses
 * (increment it whenever the tables are rebuilt or rewritten).  The pin must not outlive the tables: dd = NULL removes it -
 * with generation != 0 only if that generation is still the one pinned (an owner releasing its own pin when its tables
 * are freed or replaced; it cannot remove a later owner's), with generation = 0 unconditionally.  The kept copy is tied
 * to the stream it was made on; a call on another stream makes its own. */
int corahip_clarray_tables_pin(corahip_ctx *ctx, const double *dd, const double *dv, const double *vv,
                               uint64_t generation);

/* the bare aps callable at n independent points (corr.py:953-982): lx = log10(l), chi1, chi2,
 * and the coefficient triples b1 b2 P, (f1 b2 + f2 b1) P, f1 f2 P with P = D1 D2 pf1 pf2
 * (the 1/(xc^2 pi) factor is applied by the kernel).  All arrays [n]. */
int corahip_aps_table21cm_points(corahip_ctx *ctx, const double *dd, const double *dv, const double *vv,
                                 int nkperp, int nkpar, double kperpmin, double kperpmax, double kparmax,
                                 long n, const double *lx, const double *chi1, const double *chi2,
                                 const double *cdd, const double *cdv, const double *cvv, double *out);

/* separable model C_l = A_l * B(nu,nu') (cora/foreground/gaussianfg.py:40-41):
 *   al [nl], bcov [F*zint, F*zint] (sub-sampled frequency covariance), w [zint] -> out [nl,F,F] */
int corahip_clarray_separable(corahip_ctx *ctx, const double *al, int nl, const double *bcov, int F,
                              int zint, const double *w, double *out);

/* Romberg reduction of host-evaluated samples (skysim.py:62-67):
 *   clt [nl, F, zint, F, zint] -> out [nl, F, F] = sum_ab w_a w_b clt                */
int corahip_romb_reduce(corahip_ctx *ctx, const double *clt, int nl, int F, int zint, const double *w,
                        double *out);

/* ---- K2: per-l matrix root ---------------------------------------------------------
 * Replaces the loop body of mkfullsky (skysim.py:115-119) and
 * nputil.matrix_root_manynull(truncate=False) (cora/util/nputil.py:51-101):
 *   Cm = C_l + I * max(diag C_l) * jitter_rel;  T_l = chol_lower(Cm);  if a pivot is
 *   not positive (LAPACK potrf failure) -> symmetric eigen-decomposition, eigenvalues
 *   < max * eig_thresh set to 0, T_l = V sqrt(Lambda).
 *   C [nl,F,F] -> T [nl,F,F];  info [nl] int32: 0 = Cholesky, 1 = eigen branch.      */
int corahip_factor_batched(corahip_ctx *ctx, const double *C, int nl, int F, double jitter_rel,
                           double eig_thresh, double *T, int32_t *info);

/* ---- K3: correlated draw -----------------------------------------------------------
 * Normal stream layout ("stream order"; nputil.py:104-125 called from
 * skysim.py:120): for l = 0..lmax: F*(l+1) reals [nu'][m] then F*(l+1) imags [nu'][m];
 * total 2*F*nalm doubles.  The 1/sqrt(2) of complex_std_normal is applied by draw_alm.
 * normals_philox fills that buffer with the device stream: the elements (l, c = 0 / 1, nu', m) are the two Box-Muller
 * outputs of Philox4x32-10 counter {m, l*F + nu'} under key `seed` (independent of the GPU count; the mapping of the
 * four output words to the pair is specified in oracle/philox.py and cora_amd/csrc/rng_dev.h). */
int corahip_normals_philox(corahip_ctx *ctx, uint64_t seed, int lmax, int F, double *g);

/* The REFERENCE's own seeded stream on the device: the next n values of
 * numpy.random.Generator(PCG64).standard_normal - what `rng.standard_normal(shape)` of cora/util/nputil.py:121-125
 * returns for the `rng = default_rng(seed)` of cora/signal/lss.py:449-450 - bit for bit (fast-path and wedge samples
 * are one exact multiply; tail samples use glibc's log1p, the wedge test glibc's exp, both restated operation by
 * operation), written to g[0..n) in draw
 * order: with n = 2*F*nalm the "stream order" buffer draw_alm consumes.
 *   state, inc   host: the 128-bit PCG64 state and increment as {high 64 bits, low 64 bits}
 *                (rng.bit_generator.state["state"]["state" | "inc"])
 *   n_raw        host, out: the number of raw 64-bit draws the n normals consumed (1.0215 n on average: the ziggurat
 *                takes a data-dependent number per sample); corahip_pcg64_advance(state, inc, *n_raw) is the state
 *                numpy would be left in.
 * Synchronises the context's stream (n_raw is read back).  numpy's algorithm: PCG64 = pcg_setseq_128_xsl_rr_64,
 * 256-strip ziggurat of numpy/random/src/distributions/distributions.c; restated in oracle/npnormal.py. */
int corahip_normals_pcg64(corahip_ctx *ctx, const uint64_t host_state[2], const uint64_t host_inc[2], int64_t n,
                          double *g, uint64_t *host_n_raw);
/* numpy's Generator(PCG64).normal(0, scale[:, None], (nrow, ncol)), written or added in place: with z the next
 * nrow * ncol values of that generator's standard_normal in draw order (corahip_normals_pcg64), element (r, c) is
 *   v = 0.0 + scale[r] * z[r * ncol + c]     (one rounded multiply, then the rounded add of 0.0 - numpy's loc -, which
 *                                             gives +0.0 for scale = 0 whatever the sign of z; no contraction)
 *   out[row_off[r] + c] = v                  (accumulate = 0)     or     = out[row_off[r] + c] + v   (accumulate = 1)
 * straight out of the generator's emit pass: no buffer of normals, no second sweep over `out`.
 *   scale     device [nrow]
 *   row_off   device [nrow] element offsets into out, NULL = r * ncol.  The rows must not overlap; the CALLER checks
 *             that every row_off[r] + ncol lies inside out (the kernel cannot).
 *   host_n_raw as in corahip_normals_pcg64.  CORAHIP_ESTATE while a draw session is pending.
 * The rows are cut into sessions of about 2^28 values (each continues from corahip_pcg64_advance of the one before: the
 * bits do not depend on the cut); synchronises the context's stream once per session. */
int corahip_normal_rows_pcg64(corahip_ctx *ctx, const uint64_t host_state[2], const uint64_t host_inc[2],
                              long nrow, long ncol, const double *scale, const int64_t *row_off, double *out,
                              int accumulate, uint64_t *host_n_raw);
/* Test hook of that stream's one libm call in the accept path: y[i] = exp(x[i]) as the wedge test of the ziggurat
 * evaluates it on the device - glibc's table-driven exp (sysdeps/ieee754/dbl-64/e_exp.c) in the evaluation order of its
 * FMA build, the libm numpy's random_standard_normal calls (reached from cora/util/nputil.py:125) - for |x| < 512.
 * x, y device arrays; asynchronous on the context's stream.  tests/test_gpu_npnormal.py sweeps it against the host's exp. */
int corahip_glibc_exp(corahip_ctx *ctx, const double *x, int64_t n, double *y);
/* host arithmetic: the PCG64 state after `delta` steps (numpy's bit_generator.advance) */
int corahip_pcg64_advance(const uint64_t host_state[2], const uint64_t host_inc[2], uint64_t delta,
                          uint64_t host_out_state[2]);

/* numpy's LEGACY normal stream on the device: the next n values of np.random.standard_normal - what the reference
 * draws when it is called WITHOUT a generator (rng=None in cora/util/nputil.py:121-123; Sky3d.getsky(),
 * cora/core/maps.py:235-237): the global MT19937 state + the polar method of numpy's legacy_gauss with its one cached
 * value.  host_state: np.random.get_state(legacy=False) as a struct - key (624 words), pos, has_gauss, gauss - in; the
 * state numpy would be left in out (an equivalent (key, pos) pair: the 624-word block the generator is in and the
 * position inside it).  Which attempts of the polar method are accepted - and with it the state - is numpy's exactly;
 * the values take glibc's log restated operation by operation (its FMA build, csrc/mtlegacy.hip glibc_log_fma) and
 * correctly rounded sqrt / divisions: numpy's bit for bit where numpy's libm is that routine, within 4 ulp elsewhere.
 * Synchronises the context's stream.  Algorithm: csrc/mtlegacy.hip (MT19937 cut into segments by jump-ahead polynomials
 * over GF(2), csrc/mt_jump.inc); restated in oracle/mtlegacy.py. */
typedef struct corahip_mt_state {
    uint32_t key[624];
    int32_t pos, has_gauss;
    double gauss;
} corahip_mt_state;
int corahip_normals_mt19937_legacy(corahip_ctx *ctx, corahip_mt_state *host_state, int64_t n, double *g);

/* a_lm(nu) = sum_nu' T_l[nu,nu'] g_lm(nu')  (skysim.py:121) for channels nu0 <= nu < nu0+nnu.
 *   T [lmax+1, F, F], info [lmax+1] (from factor_batched; NULL = treat all as dense),
 *   g stream order (above), alm_dev: device a_lm layout [nalm][nnu_pad/4][2][4]
 *   (packed healpy index idx = m(2 lmax+1-m)/2 + l; channel nu0+4g+v at [g][c][v], c = re/im;
 *   nnu_pad = nnu rounded up to a multiple of 4, padding channels are written as 0).  */
int corahip_draw_alm(corahip_ctx *ctx, const double *T, const int32_t *info, const double *g, int lmax,
                     int F, int nu0, int nnu, double *alm_dev);

/* draw_alm with only the rank's rows of the factors resident: T_rows [lmax+1, nnu, F] = rows nu0 .. nu0+nnu-1 of every T_l
 * (see draw_alm_philox_rows) */
int corahip_draw_alm_rows(corahip_ctx *ctx, const double *T_rows, const int32_t *info, const double *g, int lmax,
                          int F, int nu0, int nnu, double *alm_dev);

/* draw_alm with the device stream generated in registers (same values as normals_philox(seed) followed by
 * draw_alm, without the 16*F*nalm-byte normal buffer) */
int corahip_draw_alm_philox(corahip_ctx *ctx, const double *T, const int32_t *info, uint64_t seed, int lmax,
                            int F, int nu0, int nnu, double *alm_dev);

/* draw_alm_philox with only the rank's rows of the factors resident: T_rows [lmax+1, nnu, F] holds rows
 * nu0 .. nu0+nnu-1 of every T_l (what a frequency-sharded rank receives from the all-to-all of the
 * l-sharded factor stack: 1/N of the all-gather traffic and memory).                                */
int corahip_draw_alm_philox_rows(corahip_ctx *ctx, const double *T_rows, const int32_t *info, uint64_t seed,
                                 int lmax, int F, int nu0, int nnu, double *alm_dev);

/* A rank's channels as one block or as the two chunks of a FOLDED frequency shard: local channel c < chunk_nnu is global
 * channel nu0[0] + c, local channel chunk_nnu + c is nu0[1] + c (nchunks = 2; nu0[1] >= nu0[0] + chunk_nnu; chunk_nnu a
 * multiple of 4; F even).  The draw's cost grows with the channel index (T_l is lower triangular: channel nu takes nu + 1
 * terms), so a frequency shard made of a low and a high chunk - rank r of N takes chunks r and 2 N - 1 - r of 2 N - costs
 * every rank the same (cora_amd.parallel, `fold=True`; the reference's contiguous split, cora/core/skysim.py:132-134,
 * stays the default).  T_rows [lmax+1, nchunks * chunk_nnu, F] holds the rows of the local channels in local order;
 * alm_dev and the maps made from it are in local order too. */
typedef struct corahip_chanset {
    int32_t nchunks, chunk_nnu;
    int32_t nu0[2];
} corahip_chanset;
int corahip_draw_alm_philox_rows_set(corahip_ctx *ctx, const double *T_rows, const int32_t *info, uint64_t seed,
                                     int lmax, int F, const corahip_chanset *set, double *alm_dev);

/* ---- the whole of skysim.mkfullsky in one call (cora/core/skysim.py:72-136, single process) --------------------
 * C [L, F, F] (device; L = lmax + 1 of `plan`) -> maps of channels nu0 .. nu0+nnu-1: jitter + root per l (:115-119),
 * complex normals (:120), a_lm = T_l g_l (:121), HEALPix synthesis (:130).  A chain of the entry points above
 * (factor_batched, normals_pcg64 / draw_alm*, alm2map) on buffers cut from ONE caller-owned device workspace.
 *   rng   which normals (host struct):
 *           CORAHIP_RNG_PCG64   the reference's seeded call, rng = numpy.random.default_rng(seed): `state`, `inc` are
 *                               bit_generator.state["state"]["state" | "inc"] as {high, low} 64-bit words; numpy's
 *                               sequence is continued on the device and `state` is UPDATED to the state numpy would be
 *                               left in (the call synchronises the stream for that);
 *           CORAHIP_RNG_STREAM  `stream`: DEVICE pointer to 2 F nalm normals in stream order (any generator, drawn by
 *                               the caller in the reference's order - e.g. rng=None, numpy's legacy global state);
 *           CORAHIP_RNG_MT19937 the reference called WITHOUT a generator (rng=None: numpy's legacy global state, what
 *                               Sky3d.getsky() draws from): `legacy` points to np.random.get_state(legacy=False) as a
 *                               corahip_mt_state; continued on the device (corahip_normals_mt19937_legacy) and UPDATED;
 *           CORAHIP_RNG_PHILOX  the library's counter-based stream under `seed` (not numpy's numbers).
 *   alms  0: out = maps [nnu, npix] RING (skysim.py:130-136);  1: out = a_lm [nnu, 1, L, L] complex128, m > l zero (:123-125)
 *   workspace  >= corahip_mkfullsky_workspace_bytes(...) for one synthesis pass; a smaller one (down to the factors,
 *              the a_lm and one 8-channel synthesis chunk) is worked through in chunks; the PCG64 / MT19937 kinds draw
 *              through corahip_draw_alm_numpy (below): their normals live in the library's own ring, range by range;
 *              CORAHIP_ENOMEM with the sizes in corahip_last_error() below that.                                      */
#define CORAHIP_RNG_STREAM 0
#define CORAHIP_RNG_PHILOX 1
#define CORAHIP_RNG_PCG64 2
#define CORAHIP_RNG_MT19937 3
typedef struct corahip_rng {
    int32_t kind, reserved;
    const double *stream;
    uint64_t seed;
    uint64_t state[2], inc[2];
    corahip_mt_state *legacy;
} corahip_rng;
int corahip_mkfullsky_workspace_bytes(const corahip_sht_plan *plan, int F, int nu0, int nnu, int rng_kind, int alms,
                                      size_t *bytes);
int corahip_mkfullsky(corahip_ctx *ctx, const corahip_sht_plan *plan, const double *C, int F, corahip_rng *host_rng,
                      int nu0, int nnu, int alms, double *out, void *workspace, size_t workspace_bytes);

/* draw_alm with numpy's OWN normal stream generated on the device RANGE BY RANGE, as the reference consumes it inside its
 * l loop (cora/core/skysim.py:114-121, cora/util/nputil.py:121-125): normals_pcg64 / normals_mt19937_legacy followed by
 * draw_alm (rows = 0: T [lmax+1, F, F]) or draw_alm_rows (rows = 1: T_rows [lmax+1, nnu, F]), bit for bit, WITHOUT the
 * 16 F nalm-byte stream buffer (8.6 GB at F = 256, lmax = 2048; 137 GB at F = 1024, lmax = 4096): the generator's
 * count + scan passes cover the whole stream, its emit pass fills one slot of a two-slot ring (library-owned, ring_bytes
 * in total, 0 = the default: 2 GiB - the measured optimum of the whole step at F = 256, lmax = 2048 - while the
 * stream is <= 1/8 of the device memory, else 1/16 of the memory, or CORAHIP_RING_MB; a slot is never smaller than the normals of l = lmax) per range
 * of multipoles on a second stream while K3 consumes the other slot.
 *   host_rng  (the struct of corahip_mkfullsky above) kind CORAHIP_RNG_PCG64 (state, inc as in corahip_normals_pcg64) or CORAHIP_RNG_MT19937 (legacy state);
 *             UPDATED to the state numpy would be left in.  Synchronises the context's stream (that read-back).
 * _begin / _end: the same in two halves.  _begin enqueues everything and returns without waiting; the caller goes on
 * enqueueing (the synthesis of the a_lm) and calls _end when it wants the generator state: _end waits for the context's
 * stream, updates host_rng and frees `pending`.  Between the two, no other numpy-stream draw may be started on the
 * context (enforced: a second _begin, corahip_normals_pcg64 and corahip_normals_mt19937_legacy return CORAHIP_ESTATE
 * while a session is pending - they share its device tables) and host_rng->legacy (MT19937 kind) must stay valid. */
typedef struct corahip_draw_pending corahip_draw_pending;
int corahip_draw_alm_numpy(corahip_ctx *ctx, const double *T, int rows, const int32_t *info, corahip_rng *host_rng,
                           int lmax, int F, int nu0, int nnu, double *alm_dev, size_t ring_bytes);
int corahip_draw_alm_numpy_begin(corahip_ctx *ctx, const double *T, int rows, const int32_t *info, const corahip_rng *host_rng,
                                 int lmax, int F, int nu0, int nnu, double *alm_dev, size_t ring_bytes,
                                 corahip_draw_pending **pending);
int corahip_draw_alm_numpy_end(corahip_ctx *ctx, corahip_draw_pending *pending, corahip_rng *host_rng);
/* _begin in its two halves.  _prepare is the part of a draw that does NOT depend on the factors - ranges, ring, the
 * generator's own passes (count + scan / jump tree + count) and the emit passes of the first two ranges, all on the
 * library's generator stream: a caller that issues it BEFORE the launches that make the factors (C_l integration,
 * factorisation) lets the generator run beside them (the stream is a function of the generator alone; the reference draws
 * it inside mkfullsky, cora/util/nputil.py:121-125, but nothing it draws depends on the covariance).  _run enqueues K3 of
 * every range against the factors (T full [L, F, F] with rows = 0 - `set` then names one block - or the row block of the
 * set's channels with rows = 1) and the remaining emit passes; _end as above.  _begin = _prepare + _run.
 * Ownership: once _prepare has returned a session, _end and nothing else frees it - exactly one _end per session,
 * whatever _run returned.  A session that is given up (no _run) or whose _run failed (it cannot be run again) is ended the
 * same way: _end waits for both streams, frees it, returns 0 and leaves host_rng untouched.  _begin and
 * corahip_draw_alm_numpy end a session whose run failed themselves.  Every error return of these entry points leaves
 * host_rng as it was on entry. */
int corahip_draw_alm_numpy_prepare(corahip_ctx *ctx, const corahip_rng *host_rng, int lmax, int F, size_t ring_bytes,
                                   corahip_draw_pending **pending);
int corahip_draw_alm_numpy_run(corahip_ctx *ctx, corahip_draw_pending *pending, const double *T, int rows, const int32_t *info,
                               const corahip_chanset *set, double *alm_dev);
/* _begin for a channel set (the struct above; T_rows = the row block of its channels) */
int corahip_draw_alm_numpy_begin_set(corahip_ctx *ctx, const double *T_rows, const int32_t *info, const corahip_rng *host_rng,
                                     int lmax, int F, const corahip_chanset *set, double *alm_dev, size_t ring_bytes,
                                     corahip_draw_pending **pending);

/* ---- frequency sharding for callers that pass the messages themselves -----------------------------
 * The reference distributes this path with caput.mpiarray over MPI (cora/core/skysim.py:97-110: C_l and the a_lm
 * buffer split over l; :125-134: allgather / redistribute to a frequency split).  These entry points give such a
 * caller the sharded path without torch.distributed: the only exchange is ONE all-to-all of factor row blocks.
 *   shard_plan        the split both sides use: multipoles [l_lo, l_hi) (contiguous blocks of l_shard, the last
 *                     ones shorter / empty), channels [nu0, nu0 + nnu); rows_exchange = 1 iff F % world == 0 (the
 *                     row-block all-to-all applies; otherwise all-gather the [L, F, F] factor stack instead).
 *                     Pure host arithmetic - any other contiguous l split (caput's) works with pack / unpack too.
 *   factor_rows_pack  T_local [n_local, F, F] (this rank's factors, corahip_factor_batched of its C_l block) ->
 *                     send [world][l_stride][F / world][F]: slab q = the rows of rank q's channels, l rows
 *                     n_local .. l_stride - 1 zero (l_stride = the largest block of any rank: equal slabs)
 *   (caller)          all-to-all: slab q of every rank goes to rank q -> recv [world][l_stride][nnu][F], slab r
 *                     from rank r; all-gather of the info flags (int32 [n_local] each)
 *   factor_rows_unpack recv + host_counts [world <= 64] (multipoles each rank holds, in rank order) ->
 *                     T_rows [sum counts][nnu][F]: what corahip_draw_alm_philox_rows consumes
 * then corahip_draw_alm_philox_rows(T_rows, info_all, seed, lmax, F, nu0, nnu) and corahip_alm2map: every rank
 * draws from the same counter-based stream for its own channels, the a_lm are never exchanged, the maps stay
 * frequency-sharded (the reference's MPIArray.wrap(sky, axis=0), skysim.py:132-134). */
typedef struct corahip_shard {
    int32_t l_lo, l_hi;      /* this rank integrates / factors multipoles [l_lo, l_hi) */
    int32_t l_shard, l_pad;  /* padded block length (equal on all ranks), l_shard * world >= L */
    int32_t nu0, nnu;        /* this rank draws and synthesises channels [nu0, nu0 + nnu) */
    int32_t rows_exchange;   /* 1: F % world == 0, factor row blocks go by all-to-all */
    int32_t L;
} corahip_shard;
int corahip_shard_plan(int L, int F, int rank, int world, corahip_shard *out);
int corahip_factor_rows_pack(corahip_ctx *ctx, const double *T_local, int n_local, int l_stride, int F, int world,
                             double *send);
int corahip_factor_rows_unpack(corahip_ctx *ctx, const double *recv, const int32_t *host_counts, int world,
                               int l_stride, int nnu, int F, double *T_rows);

/* layout converters between alm_dev and the reference's arrays:
 *   square  [nnu, 1, L, L] complex128 as returned by mkfullsky(alms=True) (skysim.py:108-125)
 *   packed  [nnu, nalm]   complex128 healpy order, as pack_alm produces (hputil.py:124-152)  */
int corahip_alm_dev_to_square(corahip_ctx *ctx, const double *alm_dev, int lmax, int nnu, double *square);
int corahip_alm_packed_to_dev(corahip_ctx *ctx, const double *packed, int lmax, int nnu, double *alm_dev);

/* ---- K4/K5: HEALPix synthesis ------------------------------------------------------
 * Replaces hputil.sphtrans_inv_sky / sphtrans_inv_real -> healpy.alm2map
 * (cora/util/hputil.py:369-391,500-531) for nnu channels at once.                   */
int corahip_sht_plan_create(corahip_ctx *ctx, int nside, int lmax, corahip_sht_plan **plan);
/* ... with the truncation of the Legendre sums as a parameter: terms with |lambda_lm(theta)| < 2^cut_exp are dropped
 * (-1000 <= cut_exp < 0; 0 = the default, -70).  The error this leaves in a pixel is bounded by
 * 2 sum_lm |a_lm| 2^cut_exp (1.7e-21 per unit coefficient at the default - the library's own choice; what the engine
 * behind healpy.alm2map, cora/util/hputil.py:388-391, truncates is not pinned, healpy is absent): lower it for a_lm whose
 * dynamic range exceeds ~1e10; -900 keeps every term fp64 can represent (what the oracle does). */
int corahip_sht_plan_create_ex(corahip_ctx *ctx, int nside, int lmax, int cut_exp, corahip_sht_plan **plan);
int corahip_sht_plan_cut_exp(const corahip_sht_plan *plan, int *cut_exp);
int corahip_sht_plan_destroy(corahip_ctx *ctx, corahip_sht_plan *plan);
/* number of v_mfma_f64_16x16x4_f64 instructions (2048 flop each) the Legendre kernel of corahip_alm2map ISSUES
 * for one pass over nnu channels with this plan - computed from the plan's first-contributing-l tables, i.e. what
 * the SQ_INSTS_VALU_MFMA_F64 counter reads for the launch.  bench.py prices K4's roofline fraction on it. */
int corahip_sht_plan_k4_mfma_count(corahip_ctx *ctx, const corahip_sht_plan *plan, int nnu,
                                   uint64_t *mfma_instructions);
/* bytes of scratch alm2map needs to process `nnu` channels in one pass */
int corahip_alm2map_workspace_bytes(const corahip_sht_plan *plan, int nnu, size_t *bytes);
/* alm_dev [nalm][nnu_pad/4][2][4] -> maps [nnu, 12 nside^2] RING order.
 * workspace: >= corahip_alm2map_workspace_bytes(plan, nnu_chunk) for some nnu_chunk (multiple
 * of 4) <= nnu_pad; channels are processed in chunks that fit.                        */
int corahip_alm2map(corahip_ctx *ctx, const corahip_sht_plan *plan, const double *alm_dev, int nnu,
                    double *maps, void *workspace, size_t workspace_bytes);

/* ---- analysis: the quadrature pass of healpy.map2alm --------------------
 * Replaces what hputil.sphtrans_real / sphtrans_sky / sph_ps obtain from healpy.map2alm
 * (cora/util/hputil.py:195-234,460-497,607-619) for nnu channels at once:
 *   a_lm = sum_pix w_ring(pix) (4 pi / npix) map(pix) conj(Y_lm(pix))
 * maps [nnu, 12 nside^2] RING -> alm_dev [nalm][nnu_pad/4][2][4] (nnu_pad = nnu rounded up to 8).
 * ring_w: device [2 nside] quadrature weights of the north rings incl. the equator (the south mirrors
 * them; what healpy reads from weight_ring_n*.fits for use_weights=True), NULL = uniform.
 * healpy's iter=N refinement alm += A(map - S alm) is composed by the caller from alm2map/map2alm. */
int corahip_map2alm_workspace_bytes(const corahip_sht_plan *plan, int nnu, size_t *bytes);
int corahip_map2alm(corahip_ctx *ctx, const corahip_sht_plan *plan, const double *maps, int nnu,
                    const double *ring_w, double *alm_dev, void *workspace, size_t workspace_bytes);

/* ---- polarisation: spin-2 synthesis ----------------------------------------
 * Replaces the Q, U part of healpy.alm2map([T, E, B], nside) behind hputil.sphtrans_inv_real_pol
 * (cora/util/hputil.py:394-432):  Q +- iU = - sum_lm (a^E_lm +- i a^B_lm) (+-2)Y_lm  (Zaldarriaga & Seljak 1997).
 * alm_dev holds nnu = 2 nfreq channels interleaved (E_0, B_0, E_1, B_1, ...) in the usual layout (nnu_pad8/4 groups
 * must equal nnu_pad4/4, i.e. nnu mod 8 in {0, 5, 6, 7}); maps [nnu, npix] RING = (Q_0, U_0, Q_1, U_1, ...).
 * T (and V) go through corahip_alm2map.  Workspace: corahip_alm2map_workspace_bytes(plan, nnu).             */
int corahip_alm2map_spin2(corahip_ctx *ctx, corahip_sht_plan *plan, const double *alm_dev, int nnu,
                          double *maps, void *workspace, size_t workspace_bytes);

/* ---- spin-2 analysis ((Q, U) -> (E, B); cora/util/hputil.py:274-323 sphtrans_real_pol -> healpy.map2alm) ----
 * Composed from scalar quadrature passes (csrc/sht_polana.hip): spin2_ring_scale writes, for every field f with
 * maps (Q_f, U_f) = channels (2f, 2f+1) of maps_qu [2 nfields, npix], the six maps
 * [Q, r1 Q, r2 Q, U, r1 U, r2 U] (r1 = 1/sin^2 theta, r2 = cos theta / sin^2 theta of the pixel's ring) as channels
 * 6f .. 6f+5 of maps6; after corahip_map2alm(maps6, 6 nfields) spin2_combine forms
 *   E = -(sum_rings W Q~ - i X U~),  B = -(sum_rings W U~ + i X Q~)
 * into alm_eb_dev [nalm][gout][2][4] with (E_f, B_f) = channels (2f, 2f+1), the layout corahip_alm2map_spin2
 * consumes; alm6_dev is [nalm][g6][2][4] (g6, gout: channel groups of four, padding channels zero).  One call sequence = one quadrature pass; healpy's iter = N is
 * alm += A(map - S alm) with corahip_alm2map_spin2 as S, composed by the caller.                      */
int corahip_spin2_ring_scale(corahip_ctx *ctx, corahip_sht_plan *plan, const double *maps_qu, int nfields,
                             double *maps6);
int corahip_spin2_combine(corahip_ctx *ctx, corahip_sht_plan *plan, const double *alm6_dev, int g6, int nfields,
                          double *alm_eb_dev, int gout);
/* The same quadrature pass as ONE Legendre pass (csrc/sht_polana_native.hip, the adjoint of corahip_alm2map_spin2's
 * kernel): the ring transforms run on the 2 nfields interleaved (Q_f, U_f) channels of maps_qu as they are, and
 * W_lm, X_lm are formed inside the contraction: no scaled copies of the maps, two ring transforms per pair where the
 * composition runs six.  alm_eb_dev: [nalm][nnu_pad8(2 nfields)/4][2][4], (E_f, B_f) = channels (2f, 2f+1), rows
 * l < 2 and padding channels zero; ring_w as in corahip_map2alm.  Results are bit-identical from call to call.
 * Workspace: corahip_map2alm_spin2_workspace_bytes(plan, nfields).                                        */
int corahip_map2alm_spin2_workspace_bytes(const corahip_sht_plan *plan, int nfields, size_t *bytes);
int corahip_map2alm_spin2(corahip_ctx *ctx, corahip_sht_plan *plan, const double *maps_qu, int nfields,
                          const double *ring_w, double *alm_eb_dev, void *workspace, size_t workspace_bytes);

/* ---- K0: the 21cm lookup tables (SURVEY 8 row a4 / section 2a "K0") ------------------------------
 * Replaces the one-off setup of RedshiftCorrelation.angular_powerspectrum_fft (cora/signal/corr.py:909-942)
 * and the spline evaluation behind it (cora/util/cubicspline.pyx:126-175,254-288).
 * ps_table21cm: dd, dv = dd mu^2, vv = dd mu^4 on the [nkperp][nkpar] grid (kperp, kpar: device arrays, as numpy's
 *   logspace / linspace made them).  dd_in == NULL: dd = P(k) sinc^2(kpar freq_window / 2 pi) with P(k) a natural
 *   cubic spline, knots (x, y, y'') [nknot] on the device - loglog != 0: exp(spline(log k)) (LogInterpolater) - times
 *   exp(-k^2 / 2 kstar^2) when kstar > 0 (cora/signal/corr21cm.py:24-29).  dd_in != NULL: dd_in is dd as the host
 *   evaluated it (any other ps_vv callable); only dv and vv are made (dd may be NULL).
 * dct1_rows: scipy.fftpack.dct(x, type=1) * scale of every row of data [nrows][n], in place, as one complex DFT
 *   of length n - 1 by the prime-factor (Good-Thomas) map: n - 1 must split into at most 6 pairwise coprime prime
 *   powers <= 2048 (nkpar = 32768: 32767 = 7 * 31 * 151).  workspace: dct1_workspace_bytes(nrows, n). */
int corahip_ps_table21cm(corahip_ctx *ctx, const double *knots_x, const double *knots_y, const double *knots_y2,
                         int nknot, int loglog, double kstar, const double *kperp, int nkperp, const double *kpar,
                         int nkpar, double freq_window, const double *dd_in, double *dd, double *dv, double *vv);
int corahip_dct1_workspace_bytes(long nrows, int n, size_t *bytes);
int corahip_dct1_rows(corahip_ctx *ctx, double *data, long nrows, int n, double scale, void *workspace,
                      size_t workspace_bytes);

/* ---- xi(r) -> C_l(chi, chi') ----------------------------------------------
 * Replaces corrfunc.corr_to_clarray (cora/signal/corrfunc.py:290-400).
 * xi_table_average: for every Gauss-Legendre node mu_m and channel pair (i, j) the radial-bin average
 *   sum_ab xw_a xw_b xi(r(mu_m, xa[i xint + a], xa[j xint + b])),  r^2 = (x - x')^2 + 2 x x' (1 - mu)
 *   (corrfunc.py:368-381) of a correlation function given as a natural cubic spline with end-slope
 *   extrapolation (cora/util/cubicspline.pyx:126-231): knots (x, y, y'') [nk],
 *   4 <= nk <= the limit xi_table_max_knots reports: the table and its look-up grid live in the LDS of every
 *   workgroup, 56 bytes per knot of the device's shared memory per workgroup (160 KB: 2925 knots); a larger table is
 *   CORAHIP_EINVAL with the limit in corahip_last_error(), before anything is launched;
 *   kind 0: spline(r); 1: exp(spline(log r)) (LogInterpolater); 2: f_t sinh(spline(asinh(r / x_t)))
 *   (SinhInterpolater).  out [nm, F, F].
 * legendre_project: out[l, n] = sum_m wt[m] P_l(mu[m]) xi[m, n], l = 0..lmax (corrfunc.py:387-397, where
 *   wt = w 4 pi / wsum); xi [nm, ncol], out [lmax+1, ncol]: Legendre matrix by recurrence + FP64 MFMA GEMM. */
int corahip_xi_table_max_knots(corahip_ctx *ctx, int *max_knots);
int corahip_xi_table_average(corahip_ctx *ctx, const double *knots_x, const double *knots_y,
                             const double *knots_y2, int nk, int kind, double x_t, double f_t,
                             const double *mu, int nm, const double *xa, const double *xw, int F, int xint,
                             double *out);
int corahip_legendre_project(corahip_ctx *ctx, const double *mu, const double *wt, int nm, int lmax,
                             const double *xi, long ncol, double *out);

/* xi_multi_average: the radial-bin average of xi_table_average for nfun (1 to 4) tables at once that share their knots
 *   knots_x [nk], their kind and x_t; knots_y, knots_y2 [nfun, nk] and f_t [nfun] (host memory) are per table.  The
 *   separation, the abscissa and the interval are found once per (node, i, j >= i, a, b), then nfun splines are
 *   evaluated with the arithmetic of xi_table_average.  The tables are read from global memory through the caches
 *   (a prologue kernel writes one record per interval and the look-up grid into context scratch): 4 <= nk <= 2^24,
 *   no limit from LDS.  out [nm_rows, nfun, F (F + 1) / 2]: the upper triangle (i, j >= i) row-major; nm_rows >= nm, rows
 *   nm .. nm_rows - 1 are written as zeros (nm_rows a multiple of 16 and zero weights for those rows let
 *   legendre_project take the buffer as its operand without a padded copy).
 * cl_blocks: packed projection output -> full symmetric blocks, each value written to its mirror positions from one
 *   register.  nfun = 1: packed [L, npair] -> out [L, F, F].  nfun = 3: packed [L, 3, npair] with slots (0 delta delta,
 *   1 phi delta, 2 phi phi) -> out [L, 2F, 2F] with phi phi at [:F, :F], delta delta at [F:, F:] and phi delta at both
 *   off-diagonal blocks (cora/signal/lss.py:441-445).  Any other nfun is CORAHIP_EINVAL. */
int corahip_xi_multi_average(corahip_ctx *ctx, const double *knots_x, const double *knots_y,
                             const double *knots_y2, int nk, int nfun, int kind, double x_t, const double *f_t,
                             const double *mu, int nm, const double *xa, const double *xw, int F, int xint,
                             int nm_rows, double *out);
int corahip_cl_blocks(corahip_ctx *ctx, const double *packed, long L, int nfun, int F, double *out);

/* ---- xi(pi, sigma; z1, z2) (csrc/rsdcorr.hip) -------------------------------------------------
 * The flat-sky redshift-space correlation function of cora/signal/corr.py:274-348 at n points:
 *   r = sqrt(pi^2 + sigma^2), mu = pi / (r + 1e-100), the nfun natural cubic splines on the shared knots knots_x [nk]
 *   (knots_y, knots_y2 [nfun][nk]; all three on the device) at r - one interval search for all of them, the arithmetic
 *   of xi_table_average kind 0, end-slope extrapolation below knots_x[0] and from knots_x[nk - 1] on - then
 *     out = ((c0 dd0 + 2/3 c1 dv0 + 1/5 c2 vv0) - (4/3 c1 dv2 + 4/7 c2 vv2) P_2(mu) + 8/35 c2 vv4 P_4(mu)) c3.
 *   nfun = 3: tables vv0 vv2 vv4, and dd0 = dv0 = vv0, dv2 = vv2.  nfun = 6: + dd0 dv0 dv2.  Any other nfun, nk < 4 or
 *   nk > 2^24, ncoef < 1: CORAHIP_EINVAL.  coef [ncoef][4] (device) holds the rows (c0, c1, c2, c3) = (b1 b2,
 *   (b1 f2 + b2 f1) / 2, f1 f2, D1 D2 pf1 pf2); point i reads row i % ncoef.  The tables are read through the caches from
 *   interval records in context scratch (slot 12), rebuilt by every call; no LDS table.  One writer per element, no
 *   atomics, the same bits from call to call; nothing is allocated once the scratch slot has its size. */
int corahip_xi_rsd(corahip_ctx *ctx, const double *knots_x, const double *knots_y, const double *knots_y2, int nk,
                   int nfun, const double *pi, const double *sigma, long n, const double *coef, long ncoef,
                   double *out);

/* ---- P(k) -> xi(r) (csrc/pk2xi.hip) --------------------------------------------------------
 * The numerical halves of corrfunc.ps_to_corr (cora/signal/corrfunc.py:72-84, 150-264).
 * sinc_romb:     out[j] = dlk romb_i(g[i] sinc(ka[i] r[j])) over the 2^k + 1 samples i, 1 <= k <= 24, unit spacing
 *                (scipy.integrate.romb as _corr_direct uses it; the caller passes g = P(ka) ka^3 / 2 pi^2).
 *                sinc(0) = 1; nothing of size nr x 2^k is stored; a repeated call returns the same bits.
 * fftlog_phase:  u[m] = exp(i (eta ln 2 + 2 Im lnGamma((mu + 1 + i eta) / 2))), eta = 2 pi m / L, m = 0 .. N / 2
 *                (complex [N / 2 + 1]): the FFTLog kernel at q = 0.  mu > -1, L > 0.
 * logconv:       data <- irfft(rfft(data) u) in place for a real signal of length N = N1 N2 held as complex
 *                [N] (imaginary parts zero on entry, rounding residue on return); u complex [N / 2 + 1].  A unit
 *                factor means one line transform each way (N <= 4096); otherwise the four-step scheme on the
 *                [N1, N2] view, both factors <= 4096.
 * logconv_split: a split logconv takes: (N, 1) for N <= 4096, else the cheapest pair of divisors, both <= 4096;
 *                CORAHIP_EINVAL when there is none (N has a prime factor above 4096, or N > 4096^2).  No GPU needed. */
int corahip_sinc_romb(corahip_ctx *ctx, const double *g, const double *ka, int k, double dlk, const double *r,
                      int nr, double *out);
int corahip_fftlog_phase(corahip_ctx *ctx, double mu, double L, int64_t N, double *u);

/* jl_romb: the direct integral of sinc_romb for the orders l = 0, 2, 4 and nspec (1 to 3) integrands in one pass:
 *   out[s][i][j] = dlk romb_n(g[s][n] j_{2i}(ka[n] r[j])), g [nspec][2^k + 1], out [nspec][3][nr] (device), 1 <= k <= 24.
 *   lmask [nspec] (host): bit i set = order 2 i wanted; a slot whose bit is clear is written as +0.0.  x = ka r is
 *   rounded once, its sine and cosine are computed once and shared by the orders and the integrands.  The l = 0 slot
 *   has the bits of sinc_romb for the same g.  j_2, j_4: closed forms in sin / cos from x = 2 (4) on, the ascending
 *   series below (11 and 13 terms): absolute error of one evaluation below 9.75 (14.7) x 2^-52.  r = 0 gives
 *   dlk romb(g) for l = 0 and +0.0 for l = 2, 4.  Structure and summation order are sinc_romb's: a function of k alone,
 *   a repeated call returns the same bits, nothing of size nr x 2^k is stored. */
int corahip_jl_romb(corahip_ctx *ctx, const double *g, int nspec, const int *lmask, const double *ka, int k,
                    double dlk, const double *r, int nr, double *out);
int corahip_logconv(corahip_ctx *ctx, double *data, const double *u, int64_t N, int N1, int N2);
int corahip_logconv_split(int64_t N, int *N1, int *N2);

/* ---- flat-sky Gaussian fields (flat-sky half) ------------------------------
 * n-dimensional FFTs over C-contiguous device arrays, complex = interleaved (re, im) float64; every
 * transformed axis has length <= 4096, any length (powers of two directly, others by Bluestein).
 * fft_c2c:   in-place transform of one axis; inverse = 0: sum x e^{-2 pi i jk/n}; 1: e^{+...} / n
 *            (numpy.fft.fft / ifft along `axis`).
 * irfftn:    numpy.fft.irfftn over the LAST naxes axes (cora/util/fftutil.py:80-87 with naxes = ndim;
 *            the ifft + irfft of cora/foreground/gaussianfg.py:82-84 with naxes = 2): spec has shape
 *            rdims with the last axis rdims[-1]/2 + 1 and is OVERWRITTEN; out has shape rdims.
 * rfftn:     numpy.fft.rfftn over the last naxes axes (fftutil.py:64-77); in real rdims, spec as above.
 * randomfield_draw: spec[e] = (g1 + i g2) kweight[e] with (g1, g2) the two Box-Muller normals of
 *            Philox4x32-10 counter e under key = seed - the device form of
 *            RandomField.getfield's `randn + 1j randn` (cora/core/gaussianfield.py:115-116); count
 *            complex elements.  Follow with irfftn for the field.
 * fg_mix:    out[f, m] = aff[m] sum_c freq_weight[f, c] normals[c, m]  (complex [F, M]; aff complex [M],
 *            normals real [ncorr, M]) - the tensordot of ForegroundMap.getfield
 *            (cora/foreground/gaussianfg.py:79-82); follow with irfftn(naxes = 2).                 */
int corahip_fft_c2c(corahip_ctx *ctx, double *data, int ndim, const int64_t *dims, int axis, int inverse);
int corahip_irfftn(corahip_ctx *ctx, double *spec, int ndim, const int64_t *rdims, int naxes, double *out);
int corahip_rfftn(corahip_ctx *ctx, const double *in, int ndim, const int64_t *rdims, int naxes, double *spec);
int corahip_randomfield_draw(corahip_ctx *ctx, const double *kweight, int64_t count, uint64_t seed,
                             double *spec);
int corahip_fg_mix(corahip_ctx *ctx, const double *freq_weight, const double *normals, const double *aff,
                   int F, int ncorr, int64_t M, double *out);
/* randomfield_draw + irfftn (all axes) in one call, the spectrum GENERATED where the first pass loads it - the same
 * values, bit for bit, without writing and re-reading the 16 bytes per element of a separate draw pass: kweight real
 * [rdims[0], ..., rdims[-1]/2 + 1], spec a workspace of that many complex elements, out real rdims.  The whole of
 * RandomField.getfield with the device stream (cora/core/gaussianfield.py:102-120).                              */
int corahip_randomfield_irfftn(corahip_ctx *ctx, const double *kweight, int ndim, const int64_t *rdims, uint64_t seed,
                               double *spec, double *out);
/* The redshift-space cube of RedshiftCorrelation.realisation / Corr21cm.getfield (cora/signal/corr.py:562-770,
 * cora/signal/corr21cm.py:241-257) on top of the transforms above:
 * spec_mul_real:   spec[e] *= weight[e] (complex x real; the mu^2 factor of corr.py:590-599), count elements.
 * cube_affine:     out[z, p] = a[z] df[z, p] + b[z] vf[z, p] + c[z] (corr.py:712-726); vf (and b) may be NULL.
 * raytrace_slices: scipy.ndimage.map_coordinates(cube, order=1, mode='constant') at the coordinates of
 *                  corr.py:744-768: out[i, ix, iy] = cube(zc[i], (tx[ix] scale[i]) / wx (n1-1) + (n1-1)/2,
 *                  (ty[iy] scale[i]) / wy (n2-1) + (n2-1)/2), 0 outside [0, n-1]; cube [n0, n1, n2],
 *                  out [numz, numx, numy].                                                         */
int corahip_spec_mul_real(corahip_ctx *ctx, double *spec, const double *weight, int64_t count);
int corahip_cube_affine(corahip_ctx *ctx, const double *df, const double *vf, const double *a, const double *b,
                        const double *c, int n0, int64_t plane, double *out);
int corahip_raytrace_slices(corahip_ctx *ctx, const double *cube, int n0, int n1, int n2, const double *zc,
                            const double *scale, const double *tx, const double *ty, double wx, double wy,
                            int numz, int numx, int numy, double *out);

/* ---- large-scale structure: Zel'dovich SPH density assignment -------------------------------
 * healpix_neighbours: out [npix, 9] int32 (npix = 12 nside^2, RING): entry 0 the pixel itself, 1..8 its
 *            neighbours in healpy.get_all_neighbours order (SW, W, NW, N, NE, E, SE, S), -1 where none exists
 *            (the nn_ind table of cora/signal/lss.py:1353-1355).  1 <= nside <= 8192.
 * za_density_sph: cora/signal/lss.py:1305-1419 (pmesh.pyx:29-279, pmesh_util.c:4-42): every voxel (ii, p) of
 *            delta_bias [nchi, npix] is a particle of mass 1 + delta_bias moved by psi [3, nchi, npix] (radial,
 *            theta, phi) from (chi[ii], centre of p); its mass is spread over the 9 pixels around its new
 *            direction x 3 radial bins with Gaussian weights of width sigma_ang (pixels) and sigma_chi (bins)
 *            x clip(1 + delta_m, 0.1, 3)^(-1/3); out [nchi, npix] is ADDED to, then 1 is subtracted from every
 *            element.  Bin ri goes to out[ri, pix] (the reference's C scatter uses a row stride of 9 instead
 *            of npix).  chi ascending, nchi >= 3 (else CORAHIP_EINVAL).  Float atomics: repeated
 *            calls agree to rounding, not bit for bit.                                                    */
int corahip_healpix_neighbours(corahip_ctx *ctx, int nside, int32_t *out);
int corahip_za_density_sph(corahip_ctx *ctx, const double *psi, const double *delta_bias, const double *delta_m,
                           const double *chi, int nchi, int nside, double sigma_ang, double sigma_chi, double *out);

/* ---- large-scale structure: the displacement field (cora/signal/lssutil.py:225-261 gradient -> healpy.alm2map_der1,
 * cora/signal/lss.py:806-828) ----------------------------------------------------------------------
 * Derivative synthesis composed around corahip_alm2map (csrc/sht_der1.hip): with x = cos theta of the ring,
 *   dT/dtheta = (x S[a1] - S[a2]) / sin theta,  (1/sin theta) dT/dphi = S[a3] / sin theta,
 *   a1_lm = l a_lm,  a2_{l-1,m} = sqrt((2l+1)/(2l-1) (l^2 - m^2)) a_lm,  a3_lm = i m a_lm.
 * der1_alm_prep: channel groups g0 .. g0 + g_in - 1 of alm_dev [nalm][g_src][2][4] -> alm3_dev [nalm][3 g_in][2][4],
 *            group blocks [a1 | a2 | a3].  The caller then runs corahip_alm2map(alm3_dev, 12 g_in channels) into
 *            maps3 [12 g_in, npix] (cut_exp of the plan as for alm2map: terms below 2^cut_exp per unit coefficient are
 *            dropped, which bounds the error of the derivative by 2 sum |l a_lm| 2^cut_exp / sin theta).
 * der1_combine: for fields f < nfields <= 4 g_in: out_theta[f] = s_theta[f] (x A - B) / sin theta and
 *            out_phi[f] = s_phi[f] C / sin^(1 + phi_extra) theta with A, B, C = rows f, 4 g_in + f, 8 g_in + f of
 *            maps3; s_theta, s_phi: device arrays of per-field factors or NULL (= 1); phi_extra 0 or 1;
 *            out_theta, out_phi [nfields, npix] each (separate, 16-byte aligned).
 * radial_gradient: numpy.gradient(f, x, axis=0) * s_r[:, None] for f [n, npix], n >= 2: row i is
 *            (a f[i-1] + b f[i]) + c f[i+1] with (a, b, c) = x_coef[i] (device [n][3]; numpy's second-order interior
 *            coefficients for non-uniform x, the one-sided pair and a 0 on the end rows); s_r device [n] or NULL;
 *            out [n, npix] must not overlap f.
 * All three return CORAHIP_EINVAL on arguments they cannot take.                                            */
int corahip_der1_alm_prep(corahip_ctx *ctx, corahip_sht_plan *plan, const double *alm_dev, int g_src, int g0, int g_in,
                          double *alm3_dev);
int corahip_der1_combine(corahip_ctx *ctx, corahip_sht_plan *plan, const double *maps3, int g_in, int nfields,
                         const double *s_theta, const double *s_phi, int phi_extra, double *out_theta, double *out_phi);
int corahip_radial_gradient(corahip_ctx *ctx, const double *f, const double *x_coef, const double *s_r, int n, long npix,
                            double *out);

/* ---- large-scale structure: bias, linear dynamics, Fingers of God, map (csrc/lsschain.hip) ------------------
 * The steps of cora/signal/lss.py around the Zel'dovich step (GenerateBiasedFieldBase.process :556-603,
 * LinearDynamics.process :862-918, FingersOfGod.process :1162-1220, BiasedLSSToMap.process :944-993) and the lssutil
 * functions they call.  All fields are row-major [n, ncol] float64 on the device, row = slice; rows need only 8-byte
 * alignment (ncol may be odd).  Every function returns CORAHIP_EINVAL on arguments it cannot take.
 * slice_mix:  out = K f for K [n, n], 1 <= n <= 4096, ncol >= 1, with FP64 MFMA; out must overlap neither f nor K.
 *            ranges: NULL, or device int32 [ceil(n / 16)][2]: for output rows 16 b .. 16 b + 15 the input slices
 *            [klo, khi) outside which every K entry of those rows is exactly zero (the kernel widens them to
 *            multiples of 4 and clips them to the matrix); products outside are not formed.  For finite f the result is
 *            the same, bit for bit, as with ranges NULL; a non-finite f in a skipped slice does not propagate.
 *            No atomics: two calls on the same inputs give identical bits.
 * slice_diff2: lssutil.diff2 along axis 0, n >= 4: d2[i] = ((c0 w0 + c1 w1) + c2 w2) + c3 w3 with
 *            (c0 .. c3) = coef[i] (device [n][4]) and w0 .. w3 = rows st .. st + 3 of f, st = min(max(i - 2, 0), n - 4);
 *            every product and sum is rounded on its own.  g, h (both or neither, [n, ncol]) with device [n] factors
 *            s, t: out = (h + s[i] g) + d2 t[i]; f NULL (then g, h, s required, any n >= 1): out = h + s[i] g.
 *            out must not overlap f; it may be g or h.
 * slice_moments: sum1[i] = sum_p (f[i ld + p] - c[i]), sum2[i] = sum_p (f[i ld + p] - c[i])^2 over p < ncol; ld >= ncol the
 *            row stride, c device [n] or NULL (= 0).  Block partials in work (slice_moments_workspace_bytes), then
 *            one ordered pass: no atomics, identical bits from call to call.
 * bias_field: out = c1[i] f + c2[i] (f f - m2[i]); c2, m2 both NULL: exactly c1[i] f.  out == f allowed.
 * lognormal: out[i ld_out + p] = ((exp(f[i ncol + p] - hv[i]) - 1) pre) rs[i], exp as glibc's (then - 1, not expm1);
 *            hv NULL: no transform (out = (f pre) rs), rs NULL: 1.  ld_out >= ncol (plane 0 of a [n, 4, ncol] map:
 *            ld_out = 4 ncol); in place (out == f, ld_out == ncol) allowed, any other overlap is not.            */
int corahip_slice_mix(corahip_ctx *ctx, const double *K, const double *f, const int32_t *ranges, int n, long ncol,
                      double *out);
int corahip_slice_diff2(corahip_ctx *ctx, const double *f, const double *coef, const double *g, const double *h,
                        const double *s, const double *t, int n, long ncol, double *out);
int corahip_slice_moments_workspace_bytes(int n, long ncol, size_t *bytes);
int corahip_slice_moments(corahip_ctx *ctx, const double *f, long ld, const double *c, int n, long ncol, void *work,
                          size_t work_bytes, double *sum1, double *sum2);
int corahip_bias_field(corahip_ctx *ctx, const double *f, const double *c1, const double *c2, const double *m2, int n,
                       long ncol, double *out);
int corahip_lognormal(corahip_ctx *ctx, const double *f, const double *hv, const double *rs, double pre, int n, long ncol,
                      long ld_out, double *out);

/* ---- spectra of a_lm (csrc/spectra.hip): the multi-frequency angular power spectrum, healpy's alm2cl for every pair ----
 * out[l, i, j] = (1 / (2l+1)) sum_{m=0..l} c_m (Re a_i(l,m) Re b_j(l,m) + Im a_i(l,m) Im b_j(l,m)), c_0 = 1, c_{m>0} = 2
 * (Im a_l0 enters as stored), out [lmax+1, nx, ny] row-major - clarray's layout, what mkfullsky takes.
 *   alm_a, alm_b  device a_lm layout [nalm][nnu_pad/4][2][4] of nx resp. ny channels, 16-byte aligned, with
 *                 nnu_pad = the channel count rounded up to a multiple of 4: what draw_alm* write and what
 *                 Context.map2alm / hputil.map2alm_device return (a raw corahip_map2alm buffer pads to 8 and has that
 *                 shape for n mod 8 in {0, 5, 6, 7}).  Padding channels are never read into out, whatever they hold.
 *   alm_b         NULL or == alm_a: the symmetric case (ny == nx); out is then bitwise symmetric in (i, j).
 * One FP64 MFMA Gram product per l; no atomics, no workspace: identical bits from call to call.  Per output the
 * 2 (l+1) products are added by FMAs in a fixed order (the m > 0 terms, doubled exactly, then m = 0), then one division.
 * out must overlap neither operand.  nx, ny >= 1, lmax >= 0. */
int corahip_alm_cross_spectra(corahip_ctx *ctx, const double *alm_a, int nx, const double *alm_b, int ny, int lmax,
                              double *out);

/* Channel gather in the same layout: channel dst_first + j of dst = channel idx[j] of src, j < n, for every (l, m) and
 * both components, bit for bit.  What puts T, E, B (and V) of a polarised sky - E and B interleaved in one buffer, T in
 * another - into one field-major operand of alm_cross_spectra without full-size temporaries.
 *   src, dst      device [nalm][G][2][4], 16-byte aligned, G = ceil(nsrc / 4) resp. ceil(ndst / 4) channel groups.  A
 *                 buffer padded to 8 channels (a raw map2alm buffer, what Context.map2alm_spin2 returns) is passed with
 *                 nsrc = 4 G, its padded channel count; its padding channels can then be indexed like any other.
 *   idx           device int32 [n], every entry in [0, nsrc); repeats are allowed.  The library cannot check device data:
 *                 an entry outside the range writes nothing for its channel (Context.alm_gather_channels refuses it on
 *                 the host).
 * Only channels [dst_first, dst_first + n) of dst are written: the other channels of the first and last group touched
 * and the padding channels keep what they held.  One writer per element, no atomics, no workspace: identical bits from
 * call to call.  16-byte stores for the pairs that lie inside the range, 8-byte stores at its ragged ends.  dst must not
 * overlap src.  n, nsrc, ndst >= 1, 0 <= dst_first <= ndst - n, lmax >= 0 (EINVAL otherwise). */
int corahip_alm_gather_channels(corahip_ctx *ctx, const double *src, int nsrc, const int32_t *idx, int n, int lmax,
                                double *dst, int ndst, int dst_first);

/* ---- HEALPix RING bilinear interpolation (csrc/hpinterp.hip): healpy.get_interp_weights / get_interp_val ------------
 * The published HEALPix scheme (get_interpol), restated: the two iso-latitude rings around theta (ring colatitudes are
 * acos of the ring z of hputil.pix2ang), on each ring the two nearest pixel centres with weights linear in phi
 * (wrapping round), between the rings weights linear in theta; north of the first / south of the last ring the pole is
 * a virtual sample, the mean of the 4 pixels of that ring.  theta in [0, pi]; phi is taken mod 2 pi.  Every returned or
 * touched pixel index lies in [0, npix) whatever theta and phi hold.  1 <= nside <= 8192, any nside.
 * healpix_interp_weights: theta, phi [n] -> pix_out int64 [4][n], w_out [4][n]: the upper ring's two pixels, then the lower
 *            ring's; past the first ring the upper pair is the opposite pair (p + 2) & 3 of ring 1 with weight
 *            (1 - wt) / 4 each (ring 1's own pair: w wt + (1 - wt) / 4), mirrored past the last ring.
 * healpix_interp_val: maps [nmap][npix] -> out [nmap][n], out[m][q] = sum_k w_k maps[m][pix_k]; weights computed once per
 *            query.  No atomics: identical bits from call to call.
 * healpix_rotate_maps: out[m][p] = interp(maps[m], R n_p) for the centre n_p of every output pixel; R a HOST double[9],
 *            row major.  Fused: no theta / phi arrays.  out must not overlap maps (CORAHIP_EINVAL).
 * za_density_grid: cora/signal/lss.py:996-1096: every voxel (ii, p) of delta_bias [nchi, npix] is a particle of mass
 *            1 + delta_bias moved by psi [3, nchi, npix] exactly as in za_density_sph; its mass goes to the 4
 *            interpolation pixels of its new direction x the 2 radial bins around its new distance (chi extended by one
 *            extrapolated cell at each end, np.digitize, weights |chi1 - x| / dchi and |x - chi0| / dchi); a bin outside
 *            [0, nchi) drops its share.  out [nchi, npix] is ADDED to, then 1 is subtracted from every element.  Bin ri
 *            goes to out[ri, pix] (the reference's C scatter uses a row stride of 4 instead of npix).
 *            chi ascending, nchi >= 2.  Global f64 atomics: repeated calls agree to rounding, not bit for bit.          */
int corahip_healpix_interp_weights(corahip_ctx *ctx, int nside, const double *theta, const double *phi, long n,
                                   int64_t *pix_out, double *w_out);
int corahip_healpix_interp_val(corahip_ctx *ctx, const double *maps, long nmap, int nside, const double *theta,
                               const double *phi, long n, double *out);
int corahip_healpix_rotate_maps(corahip_ctx *ctx, const double *maps, long nmap, int nside, const double *R, double *out);
int corahip_za_density_grid(corahip_ctx *ctx, const double *psi, const double *delta_bias, const double *chi, int nchi,
                            int nside, double *out);

/* Polarised galactic emission: the body of ConstrainedGalaxy.getpolsky (cora/foreground/galaxy.py:209-344) behind its
 * random maps (csrc/faraday.hip).  Complex arrays are interleaved (re, im) float64, 16-byte aligned.
 * complex_variance: chunk_var (galaxy.py:58-83) of a complex array: with m = mean(y), out2[0] = sum |y - m|^2 / count,
 *            out2[1..2] = m (device).  Block partials, then one ordered pass, for the mean and again for the squares: no
 *            atomics, identical bits from call to call.
 * faraday_mix: y [ncol, nphi] complex (the depth cube after the inverse FFT, unweighted), phi [nphi] the depth grid,
 *            sigma [ncol] > 0, A [nfreq, nphi] complex (the transpose of the reference's pta), scale = 1 / (2 sqrt(var)):
 *              w[p, k] = exp(-0.25 (phi[k] / sigma[p])^2) / sum_k' exp(-0.25 (phi[k'] / sigma[p])^2)      (:288-292)
 *              z[f, p] = scale sum_k A[f, k] w[p, k] y[p, k]                                              (:286, :295, :313)
 *              P[f, p] = z tanh|z| / |z|, 0 where z = 0 (the reference gives NaN there)                   (:319-320)
 *            intensity [nfreq, ncol] given: out [nfreq, 4, ncol] = (intensity, Re P intensity, Im P intensity, 0)
 *            (:324-331); NULL: out complex [nfreq, ncol] = P.  FP64 MFMA, M = channel, N = column, K = depth; weighting,
 *            saturation and the product with intensity are the operand prologue and the epilogue of the one kernel.
 *            nphi even, >= 2; nfreq, ncol >= 1.  out must not overlap an input.  No atomics, fixed sum order.
 * faraday_pack: maps [2 nchunk, npix] real (rows 2 j, 2 j + 1: real and imaginary part of depth channel k0 + j) into
 *            y[p, k0 + j] of the complex [npix, nphi] cube; k0 + nchunk <= nphi.                                        */
int corahip_complex_variance(corahip_ctx *ctx, const double *y, long count, double *out2);
int corahip_faraday_mix(corahip_ctx *ctx, const double *y, long ncol, int nphi, const double *phi, const double *sigma,
                        const double *A, int nfreq, double scale, const double *intensity, double *out);
int corahip_faraday_pack(corahip_ctx *ctx, const double *maps, int nchunk, long npix, int k0, int nphi, double *y);

/* Extra-galactic point sources (cora/foreground/pointsource.py; csrc/pointsource.hip).
 * pointsource_population: the synthetic population of PointSourceModel.getsky (:213-243) in one launch.  Source i draws
 *            from two Philox4x32-10 blocks that depend on (seed, i) alone, A = counter (i lo, i hi, 0, 0x50535243) and
 *            B = counter (i lo, i hi, 1, 0x50535243), key = seed (the a_lm and flat-sky streams use counter words 2, 3 = 0,
 *            so the streams share no block):
 *              u1 = (A0 2^21 + (A1 >> 11)) 2^-53,  u2 = (A2 2^21 + (A3 >> 11)) 2^-53,  z = first Box-Muller normal of B
 *              flux[i] = flux_min exp(spline(u1)),  index[i] = spectral_mean + spectral_width z,
 *              pix[i] = min((int64)(u2 npix), npix - 1)
 *            spline: the natural cubic spline of cora_amd.util.cubicspline.Interpolater through (knots, values) with
 *            second derivatives `second` (nknots each; knots ascending from 0 to 1: the inverse CDF of poisson.py:196-206),
 *            bisection for the last knot <= u1, then the cubic of that interval.  interval: NULL, or int32 [n] receiving
 *            that knot's index, and spline_value: NULL, or float64 [n] receiving spline(u1) (test hooks).
 * pointsource_paint: sources sorted by pixel (pix ascending, int64 [n], every value in [0, npix)) into out [nfreq, npol, npix],
 *            npol 1 or 4.  With T(i, f) = flux[i] exp(beta[i] x[f] + gamma[i] x[f]^2) (gamma NULL: no quadratic term),
 *              out[f, 0, p] (+)= ((sum over the sources i of pixel p of T(i, f)) 1e-26 c2) / den[f]
 *            and, with polw [n, 2] given (npol 4), planes 1 and 2 the same sums of T polw[i, 0] and T polw[i, 1].
 *            accumulate 0: every element of out is written (pixels without a source, plane 3, and planes 1, 2 without
 *            polw: 0).  accumulate 1: the sums are added to the occupied pixels, nothing else is touched.  One writer per
 *            element, a pixel's sources summed in ascending order of i (more than 16 of them: lane l of a wave sums sources
 *            l, l + 64, ..., then a fixed butterfly): no atomics, the same bits from call to call and for any subset of
 *            channels.  n < 2^31.  x = log(freq / pivot), den = 2 k_B nu^2 1e12 pxarea and c2 = c^2 come from the host.
 * polarise_rotate: the end of PointSourceModel.getpolsky (:258-276): intensity [nfreq, npix], qfrac, ufrac [npix] ->
 *            out [nfreq, 4, npix] = (I, Re P, Im P, 0), P = I (qfrac + i ufrac) exp(-2i wv[f] rm[p]); rm NULL: no rotation.
 * faraday_rotate: faraday_rotate (:21-51) in place on planes 1, 2 of polmap [nfreq, npol, npix], npol >= 3.
 *            In both the angle is -2 wv rm with wv = 1e-6 c / freq, the wavelength and not its square, as the reference
 *            has it (:43-45).
 * healpix_ud_grade: healpy.ud_grade(power = None) of maps [nmap, npix_in], RING in and out, nside_in and nside_out powers of
 *            two: the arithmetic mean of the 4^k children (summed pairwise in NESTED order) when degrading, replication when
 *            upgrading; no UNSEEN handling.  out [nmap, npix_out] must not overlap maps.  One thread walks the 4^k children of its
 *            pixel, so nside_in <= 64 nside_out (EINVAL beyond): degrade further in two calls.  nfreq <= 65535 in the two
 *            rotation entry points (one grid row per channel).                              */
int corahip_pointsource_population(corahip_ctx *ctx, uint64_t seed, long n, const double *knots, const double *values,
                                   const double *second, int nknots, double flux_min, double spectral_mean,
                                   double spectral_width, long npix, int64_t *pix, double *flux, double *index,
                                   int32_t *interval, double *spline_value);
int corahip_pointsource_paint(corahip_ctx *ctx, long n, const int64_t *pix, const double *flux, const double *beta,
                              const double *gamma, const double *polw, const double *x, const double *den, double c2,
                              int nfreq, int npol, long npix, int accumulate, double *out);
int corahip_polarise_rotate(corahip_ctx *ctx, const double *intensity, const double *qfrac, const double *ufrac,
                            const double *rm, const double *wv, int nfreq, long npix, double *out);
int corahip_faraday_rotate(corahip_ctx *ctx, double *polmap, const double *rm, const double *wv, int nfreq, int npol,
                           long npix);
int corahip_healpix_ud_grade(corahip_ctx *ctx, const double *maps, long nmap, int nside_in, int nside_out, double *out);

/* ---- constrained galaxy (cora/foreground/galaxy.py:43-55, :109-111, :147-207; csrc/galaxy.hip) ------------------------
 * All FP64, no atomics, one writer per element: the same bits from call to call.  Maps are [nmap, npix] row-major.
 * healpix_reorder: healpy.reorder between RING and NESTED for nside a power of two up to 8192; r2n != 0: maps in RING order
 *            -> out in NESTED order, r2n == 0: the other way.  A gather, out[i, q] = maps[i, p(q)], with the pixel map computed
 *            in the kernel (NESTED pixel = face nside^2 + the bits of x on the even places and of y on the odd ones, Gorski et
 *            al. 2005 section 4.1).  out must not overlap maps.
 * healpix_block_variance: map_variance (:43-55) without its two reordered copies: out[i, P], P a RING pixel at nside_out, is
 *            numpy's var (ddof 0) of the (nside_in / nside_out)^2 children of P in maps[i] (RING, nside_in).  Two passes, the
 *            mean and then the mean of the squared deviations, both summed over the balanced binary tree of the NESTED child
 *            order (healpix_ud_grade's tree): a block of equal values has variance exactly 0, and nside_out = nside_in gives
 *            zeros.  Up to 16 children a lane owns an output pixel, from 64 a wave does; the bits do not depend on which.
 *            nside_in <= 64 nside_out (EINVAL beyond).  out [nmap, npix_out] must not overlap maps.
 * alm_scale_l: out = alm fl[channel, l] for a_lm in the device layout [nalm][ceil(nnu / 4)][re, im][4] (packed index
 *            m (2 lmax + 1 - m) / 2 + l) and fl [nnu, lmax + 1] real: what healpy.smoothing / almxfl do between analysis and
 *            synthesis, for all channels at once.  One multiply per component: the host product, bit for bit.  The padding
 *            channels of the last group are copied.  out == alm (in place) is allowed, a partial overlap is not.
 * galaxy_combine: the end of ConstrainedGalaxy.getsky (:181-198) in one launch.  fg, fgs [nchan, npix]; haslam, sc, am [npix];
 *            lnr [nchan] = log(efreq / 408) from the host; inv_mv = 1 / mv.  For c >= skip:
 *              S = haslam[p] exp(sc[p] lnr[c]),  x = ((am[p] inv_mv) (fg[c, p] - fgs[c, p])) / S,
 *              out[c - skip, p] = S (1 + (x < 0 ? tanh(x) : x)),
 *            every operation rounded once, in this order (no contraction); exp is glibc's (< 1 ulp, |sc lnr| < 512 is the
 *            caller's to ensure), tanh the device library's.  haslam must be positive (not checked here).  npix even, all
 *            map pointers 16-byte aligned; out [nchan - skip, npix] must not overlap an input.                        */
int corahip_healpix_reorder(corahip_ctx *ctx, const double *maps, long nmap, int nside, int r2n, double *out);
int corahip_healpix_block_variance(corahip_ctx *ctx, const double *maps, long nmap, int nside_in, int nside_out, double *out);
int corahip_alm_scale_l(corahip_ctx *ctx, const double *alm, int lmax, int nnu, const double *fl, double *out);
int corahip_galaxy_combine(corahip_ctx *ctx, const double *fg, const double *fgs, const double *haslam, const double *sc,
                           const double *am, double inv_mv, const double *lnr, int nchan, int skip, long npix, double *out);

/* ---- mkconstrained (cora/core/skysim.py:139-201; csrc/constrained.hip) -------------------------------------------------
 * All FP64, no atomics, fixed reduction orders: the same bits from call to call.
 * eig_top_batched: the k algebraically largest eigenpairs of every symmetric C[l] (C [nl, F, F], the lower triangle is
 *            read): V [nl, F, k] with orthonormal columns in ascending eigenvalue order, as scipy.linalg.eigh(C[l])[1][:, -k:],
 *            theta [nl, k] their eigenvalues, info [nl]: 0 = block orthogonal iteration (16 columns, FP64 MFMA products,
 *            Rayleigh-Ritz by Jacobi in LDS), 1 = full Jacobi decomposition.  The iteration stops when every one of the k
 *            pairs has |C v - theta v|_2 <= 8 F 2^-53 |C|_inf; a block that has not got there after max_iter products
 *            (max_iter <= 0: the library's default), or whose negative eigenvalues outweigh the wanted ones, takes the
 *            full decomposition.  1 <= k <= min(8, F); F up to the limit eig_top_max_f reports (two F x 16 blocks in the
 *            LDS of a workgroup), EINVAL beyond.  The outputs must not overlap C or each other.  Synchronises the stream.
 * constrained_weights: W[l] = V[l] (V[l][f_ind, :])^-1 ([nl, F, k]) by LU with partial pivoting; W[0] = 0 and V[0] is not
 *            read (:191-192).  f_ind: k HOST indices into 0 .. F - 1 (EINVAL outside).  info [nl]: 0, or 2 where a pivot is
 *            exactly zero (scipy's solve raises there) - for every l >= 1 when f_ind names a channel twice; W[l] is NaN then.
 * alm_mix_l: alm_out[f, lm] = sum_j W[l, f, j] alm_in[j, lm], j ascending, for a_lm in the device layout
 *            [nalm][ceil(n / 4)][re, im][4] (n = k channels in, F out; packed index m (2 lmax + 1 - m) / 2 + l) and
 *            W [lmax + 1, F, k].  The padding channels of the input are not used, those of the output are written as 0.
 *            alm_out must not overlap an input; both a_lm pointers 32-byte aligned.                                    */
int corahip_eig_top_max_f(corahip_ctx *ctx, int *max_f);
int corahip_eig_top_batched(corahip_ctx *ctx, const double *C, int nl, int F, int k, int max_iter, double *V, double *theta,
                            int32_t *info);
int corahip_constrained_weights(corahip_ctx *ctx, const double *V, int nl, int F, int k, const int32_t *f_ind, double *W,
                                int32_t *info);
int corahip_alm_mix_l(corahip_ctx *ctx, const double *alm_in, int lmax, int k, const double *W, int F, double *alm_out);

/* ---- LOFAR diffuse synchrotron (cora/foreground/lofar.py:63-71; csrc/lofar.hip) ------------------------------------------
 * All FP64, no atomics, one writer per element, every summation order a function of the shape alone: the same bits from
 * call to call.
 * powerlaw_los: A, beta [ncol, nz] (nz contiguous: the memory of an [x_num, y_num, nz] field), x [nfreq] = ln(nu_i / nu_0):
 *              out[i, p] = sum_z (a0 + sa A[p, z]) exp(x[i] (b0 + sb beta[p, z])),   out [nfreq, ncol].
 *            The affine maps are applied on the way in (one fma each); the raw fields are not written.  Per term
 *            t = x b, e = exp(t), acc = fma(a, e, acc), z ascending from 0: the order depends on nz alone, so a channel
 *            computed alone has the bits of the same channel computed among many.  exp is glibc's (csrc/glibc_exp.h): below
 *            1 ulp, and |x (b0 + sb beta)| < 512 is the caller's to ensure.  With E = 1 that ulp bound,
 *              |out - exact| <= (nz + 2 max|x b| + 2 E + 4) 2^-53 sum_z |a_z| exp(x_i b_z).
 *            beta == A is allowed; out must not overlap an input.  nfreq, ncol, nz >= 1 (EINVAL otherwise, before any launch).
 * field_moments: f [ncol, nz] -> out3 (device): out3[0] the population standard deviation (numpy's ddof = 0) of the column sums
 *            s_p = sum_z f[p, z], out3[1] that of all elements, out3[2] = max |f|.  Two passes each, the mean and then the
 *            squared deviations, over block partials and one ordered final pass (scratch slot 10).                          */
int corahip_powerlaw_los(corahip_ctx *ctx, const double *A, const double *beta, const double *x, double a0, double sa,
                         double b0, double sb, int nfreq, long ncol, int nz, double *out);
int corahip_field_moments(corahip_ctx *ctx, const double *f, long ncol, int nz, double *out3);

/* ---- exact curved-sky C_l(z, z') (angular_powerspectrum_full of cora/signal/corr.py:777-868; csrc/fullsky.hip) -------------
 * C_l[i, j] = sum_n g_n A_l[i, n] A_l[j, n],  A_l[i, n] = sum_a cb[i, a] j_l(k_n chi[i, a]) - cf[i, a] j_l''(k_n chi[i, a]),
 * g_n = (2 / pi) w_n k_n^2 P(k_n) on one wavenumber grid k [nk]; chi, cb, cf are [F, nsub] (the sub-samples of a channel with
 * their quadrature weights folded into cb and cf).  All arrays on the device, FP64, no atomics, one writer per element, every
 * summation order fixed: the same bits from call to call.
 * sphbessel_radial: A [lmax + 1, F, ld_k] (k contiguous, ld_k >= nk; columns nk .. ld_k - 1 are written as zeros).
 *            j_l by the upward recurrence while l <= x = k chi and by a downward (Miller) recurrence started at
 *            lmax + 1 + ceil(sqrt(160 (lmax + 1))) + 30 above it, normalised at the turning point; j_l'' = (l (l - 1) / x^2 - 1)
 *            j_l + (2 / x) j_{l+1}.  x = 0: j_0 = 1, j_0'' = -1/3, j_2'' = 2/15, zeros otherwise.  Finite for every finite x >= 0;
 *            the error of j_l and of j_l'' stays within a few 1e-13 of the envelope 1 / max(x, 1) up to lmax = 3071
 *            (tests/_fullsky_oracle.py).  1 <= nsub <= 17, F <= 65535 (EINVAL otherwise, before any launch).
 * cl_gram:   C [lmax + 1, F, F] = (accumulate ? C : 0) + sum_{n < nk} g_n A[l, i, n] A[l, j, n] on FP64 MFMA; g of either
 *            sign.  Elements i <= j are computed and written to both places: C equals its transpose bit for bit.  An
 *            element's sum runs over n = 0, 1, ... in steps of 4 whatever F is: rows of a subset of the channels give the
 *            bits of the full call's sub-block.  With accumulate only the upper triangle of C is read.
 * clarray_fullsky: the k axis in chunks of nk_chunk, ascending: the table of a chunk into workspace
 *            (clarray_fullsky_workspace_bytes(lmax, F, nk_chunk)), then cl_gram, accumulating after the first chunk.     */
int corahip_sphbessel_radial(corahip_ctx *ctx, const double *k, int nk, const double *chi, const double *cb, const double *cf,
                             int F, int nsub, int lmax, long ld_k, double *A);
int corahip_cl_gram(corahip_ctx *ctx, const double *A, const double *g, int lmax, int F, int nk, long ld_k, double *C,
                    int accumulate);
int corahip_clarray_fullsky_workspace_bytes(int lmax, int F, int nk_chunk, size_t *bytes);
int corahip_clarray_fullsky(corahip_ctx *ctx, const double *k, const double *g, int nk, const double *chi, const double *cb,
                            const double *cf, int F, int nsub, int lmax, int nk_chunk, void *workspace, double *C);

/* ring geometry of the plan (host arrays of length 4 nside - 1), for tests */
int corahip_sht_plan_rings(const corahip_sht_plan *plan, int64_t *host_start, int32_t *host_nphi,
                           double *host_z, double *host_phi0);
/* ring-FFT class of every ring (host array of length 4 nside - 1), for tests and per-class reports: 0 = direct
 * transform (belt, power-of-two cap rings), else the Bluestein length the synthesis kernel of that ring runs
 * (a power of two, or 3 * 2^k for the rings whose 2 h - 1 fits it) */
int corahip_sht_plan_ring_classes(const corahip_sht_plan *plan, int32_t *host_len);
/* normalised associated Legendre values lambda_lm(cos theta_ring) the synthesis uses
 * (device recurrence incl. the polar seed table), l = m..lmax -> out [lmax-m+1] (device) */
int corahip_sht_lambda(corahip_ctx *ctx, const corahip_sht_plan *plan, int m, int ring_pair, double *out);
/* the same values as lane group kq (0..3) of the synthesis kernel forms them: zero in front of the group's entry row
 * R = m + 2 kq + 8 k >= lstart - 1, the plan's entry state there (four per (m, ring)), the recurrence behind it; equal
 * to corahip_sht_lambda from row max(R, lstart) on, and below the plan's cut before it.  For tests. */
int corahip_sht_lambda_entry(corahip_ctx *ctx, const corahip_sht_plan *plan, int m, int ring_pair, int kq, double *out);
/* its counterpart for the scalar synthesis kernel, whose lane group kq walks the contiguous rows [R_kq, R_kq + 2 T) of
 * an item (l_begin = m + ((lmin - m) & ~7), lmin the first contributing l of the ring's tile of 128 rt ring pairs,
 * T = (lmax - l_begin) / 8 + 1 macro-steps, R_kq = l_begin + 2 kq T; rt = 1: 64 and more channels per call, 2: fewer):
 * lambda from the plan's entry state of that group - in front of R_kq if R_kq >= lstart - 1, else in front of the first
 * row R_kq + 2 t >= lstart - 1 of the segment - to the segment's end, zero elsewhere -> out [lmax-m+1] (device);
 * info [4] (device) = (l_begin, T, R_kq, entry row or -1 if the group never enters).  For tests. */
int corahip_sht_lambda_segment_entry(corahip_ctx *ctx, const corahip_sht_plan *plan, int rt, int m, int ring_pair, int kq,
                                     double *out, int32_t *info);
/* the context's scratch under a poison byte, for tests that a call reads no scratch cell it has not written itself.
 * byte 0 .. 255: every scratch slot the context holds is filled with it on the context's stream (waited for), the
 * library's caches in those slots are marked invalid (the transposed K1 tables, the K1 pair list, the position lists
 * of the MT19937 jump), and from then on a slot that grows and the per-call device allocations of the eigen routes
 * (corahip_factor_batched, corahip_eig_top_batched) are filled with it when they are made.  byte < 0 ends that (the
 * default; nothing is filled).  slot_bytes [CORAHIP_DEBUG_NSCRATCH] (host, or NULL): the bytes each slot held at the
 * call.  CORAHIP_ESTATE while a draw session is pending.  No effect on any result of a correct library. */
#define CORAHIP_DEBUG_NSCRATCH 13
int corahip_debug_poison_scratch(corahip_ctx *ctx, int byte, size_t *slot_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CORAHIP_H */
