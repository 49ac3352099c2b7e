/*
 * hmgrid.h — C ABI of libhmgrid.so, the MI355X (gfx950) halo-model grid engine.
 *
 * The reference (simonsobs/hmvec) is pure Python and has NO FFI/plugin boundary:
 * its drop-in boundary is the Python class hmvec.HaloModel (hmvec/hmvec.py:75-572).
 * This header defines the C boundary a maintainer would bind with ctypes underneath
 * that class (see INTEGRATION.md for the stub).  Each entry point cites the reference
 * lines it replaces.
 *
 * Conventions
 *  - All numeric data is IEEE fp64.  Grids are C-contiguous [z][m][k], k fastest
 *    (hmvec/hmvec.py:24-31).
 *  - Pointers named d_* are DEVICE pointers obtained from hmg_malloc; pointers
 *    named h_* are host pointers.  No framework types cross this boundary.
 *  - This header is the ONE declaration of the ABI: the Python package derives its ctypes binding from it at import
 *    (hmvec_amd/_abi.py) and binds nothing by hand.  That makes the style binding: `#define HMG_<NAME> <integer>`,
 *    `typedef struct { ... } hmg_<x>;`, `int hmg_<name>(...);`, scalars int / double / size_t / long long, and every
 *    pointer parameter or field other than hmg_ctx*, void* and a pointer to one of the structs named d_* (bound as a
 *    plain address) or h_* (bound as a typed host pointer).  An unprefixed pointer or a declaration in another style
 *    fails the import, naming it.  Parameter names are what keyword calls of the Python layer go by.
 *  - Every function returns 0 on success, non-zero on failure; the message for the
 *    calling thread's last failure is returned by hmg_last_error().
 *  - All work is enqueued on the context's stream; only hmg_memcpy_h2d, hmg_memcpy_d2h, hmg_sync,
 *    hmg_elapsed_ms, hmg_graph_destroy, hmg_comm_barrier and hmg_comm_destroy block the host.
 *  - A context is bound to one GPU and is not thread-safe; use one per GPU/process.
 */
#ifndef HMGRID_H
#define HMGRID_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMG_ABI_VERSION 10

typedef struct hmg_ctx hmg_ctx;

/* ---- lifetime, memory, timing -------------------------------------------------- */
int         hmg_abi_version(void);
const char* hmg_last_error(void);
int hmg_ctx_create(int device, hmg_ctx** out);
int hmg_ctx_destroy(hmg_ctx* ctx);
/* Device blocks are recycled by size inside the context: hmg_free does not synchronise the device
 * (unless work was moved to another lane since the last synchronisation) and a stream of same-shaped
 * temporaries does not reach the driver's allocator.  Blocks are returned at hmg_ctx_destroy.      */
int hmg_malloc(hmg_ctx* ctx, size_t bytes, void** d_out);
int hmg_free(hmg_ctx* ctx, void* d_ptr);
int hmg_memcpy_h2d(hmg_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int hmg_memcpy_d2h(hmg_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);   /* blocks */
int hmg_memcpy_d2d(hmg_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int hmg_sync(hmg_ctx* ctx);                      /* waits for every lane */
/* Result hand-over without staging: a page-locked host block (allocate once, reuse) and an
 * asynchronous copy into it on the current lane; hmg_sync (or an event) completes it.  The
 * reference returns host arrays from get_power* (hmvec/hmvec.py:500-572); this is how a batch of
 * (nz,nk) spectra reaches the host in one DMA at link speed.                                      */
int hmg_host_alloc(hmg_ctx* ctx, size_t bytes, void** h_out);
int hmg_host_free(hmg_ctx* ctx, void* h_ptr);
int hmg_memcpy_d2h_async(hmg_ctx* ctx, void* h_pinned_dst, const void* d_src, size_t bytes);
/* The same towards the device (inputs of a sweep staged in a page-locked block), and the host-side wait for ONE
 * event - what a consumer of a streamed result block waits on while later passes keep running on the device
 * (hmg_sync would wait for those too).  The reference hands host arrays in and out (hmvec/hmvec.py:76-94,500-572). */
int hmg_memcpy_h2d_async(hmg_ctx* ctx, void* d_dst, const void* h_pinned_src, size_t bytes);
int hmg_event_synchronize(hmg_ctx* ctx, int slot);     /* blocks until the event last recorded in `slot` has happened */
/* Lanes: HMG_LANES HIP streams per context.  Every entry point enqueues on the CURRENT lane
 * (default 0).  Independent stages of the path (e.g. the NFW kernel and the profile-FFT kernel,
 * or the small per-(z,m) kernels) may be put on different lanes and ordered with events:
 * hmg_event_record(slot) on the producer lane, hmg_event_wait(slot) on the consumer lane.
 * hmg_memcpy_d2h, hmg_free and hmg_sync wait for all lanes.  Scratch inside the context is
 * shared: do not run the SAME entry point concurrently on two lanes.                        */
#define HMG_LANES 4
int hmg_lane_set(hmg_ctx* ctx, int lane);
int hmg_event_wait(hmg_ctx* ctx, int slot);      /* current lane waits for the event last recorded in slot */
/* HIP-event stopwatch on the context's stream: slots 0..HMG_EVENT_SLOTS-1. */
#define HMG_EVENT_SLOTS 4096
int hmg_event_record(hmg_ctx* ctx, int slot);
int hmg_elapsed_ms(hmg_ctx* ctx, int slot_start, int slot_stop, double* h_ms);     /* blocks */
/* One-shot: bracket the NEXT launch of the named kernel with event records at the two
 * slots (measurement hook for bench.py's roofline; -1,-1 clears).  For HMG_KERNEL_PROFILE_FFT
 * the bracket spans the integrand + rocFFT + interpolation launches of one hmg_profile_fft. */
#define HMG_KERNEL_POWER       0
#define HMG_KERNEL_NFW         1
#define HMG_KERNEL_PROFILE_FFT 2
#define HMG_KERNEL_COUNT       3
int hmg_bracket_next(hmg_ctx* ctx, int kernel_id, int slot_start, int slot_stop);
/* Captured steps.  Everything enqueued between hmg_graph_begin and hmg_graph_end - on lane 0 and on
 * every lane that joins through hmg_event_wait on an event recorded inside the capture - becomes one
 * HIP graph; hmg_graph_launch replays it with a single host call, independent branches running
 * concurrently.  No allocation, free or synchronisation may occur inside a capture (the calls that
 * would need one fail): run the same sequence once eagerly first.  A parameter sweep over a fixed
 * grid (the benchmark's step, an MCMC over HOD parameters held in device buffers) replays the graph. */
int hmg_graph_begin(hmg_ctx* ctx);
int hmg_graph_end(hmg_ctx* ctx, int* h_graph_id);
int hmg_graph_abort(hmg_ctx* ctx);                 /* leave capture mode after a failed call */
int hmg_graph_kernel_nodes(hmg_ctx* ctx, int graph_id, int* h_n);  /* kernel launches the captured step holds */
int hmg_graph_launch(hmg_ctx* ctx, int graph_id);  /* on the current lane */
int hmg_graph_destroy(hmg_ctx* ctx, int graph_id);

/* ---- A2: sigma^2(z, R(m)) ------------------------------------------------------
 * Replaces Cosmology.get_sigma2_R (hmvec/cosmology.py:245-269) + Wkr (:30-38).
 *   sigma2[z,m] = sum_j d_wq[j] * sPzk[z,j] * W(kq[j]*R[m])^2
 * d_wq carries the quadrature weight times k^2/(2 pi^2); the caller builds it from the
 * irregular-Simpson rule the reference uses (scipy.integrate.simpson, x given).
 * W is the Fourier top-hat with the Taylor branch for kR < taylor_switch.           */
int hmg_sigma2(hmg_ctx* ctx, int nz, int nm, int nq,
               const double* d_sPzk /*[nz][nq]*/, const double* d_kq /*[nq]*/,
               const double* d_wq /*[nq]*/, const double* d_R /*[nm]*/,
               double taylor_switch, double* d_sigma2 /*[nz][nm]*/);
/* The contraction reads P from a [k'][z] transposed, zero-padded copy (the MFMA A operand).  A caller
 * whose sPzk does not change between passes (the usual case: it is an INPUT of the path) lays it out
 * once - hmg_sigma2_layout_size doubles, hmg_sigma2_prepare - and calls hmg_sigma2_prepared, which
 * is hmg_sigma2 minus the transposition launch.  Same arithmetic, same result, bit for bit.        */
int hmg_sigma2_layout_size(int nz, int nq, size_t* h_doubles);
int hmg_sigma2_prepare(hmg_ctx* ctx, int nz, int nq, const double* d_sPzk, double* d_PT);
int hmg_sigma2_prepared(hmg_ctx* ctx, int nz, int nm, int nq, const double* d_PT,
                        const double* d_kq, const double* d_wq, const double* d_R,
                        double taylor_switch, double* d_sigma2);

/* ---- A3/A4: mass function n(z,m) and halo bias b(z,m) -----------------------------
 * Replaces get_fsigmaz/get_bh/get_nzm (hmvec/hmvec.py:133-161,178-185) and
 * tinker.f_nu/bias (hmvec/tinker.py:26-67).                                          */
#define HMG_MF_SHETH_TORMEN 0
#define HMG_MF_TINKER10     1
typedef struct {
    int    mode;               /* HMG_MF_* */
    double deltac, st_A, st_a, st_p;
    double rho_m0;             /* mean matter density today [Msun/Mpc^3] */
    int    lnm_uniform;        /* np.gradient takes its uniform-spacing branch */
    double lnm_step;           /* that spacing (only if lnm_uniform) */
} hmg_massfn_params;
int hmg_massfn(hmg_ctx* ctx, int nz, int nm, const hmg_massfn_params* h_par,
               const double* d_sigma2 /*[nz][nm]*/, const double* d_ms /*[nm]*/,
               const double* d_lnms /*[nm]*/,
               const double* d_tinker_z /*[nz][5] = alpha,beta,phi,eta,gamma at clamped z; NULL for ST*/,
               double* d_nzm /*[nz][nm]*/, double* d_bh /*[nz][nm]*/);

/* hmg_sigma2_prepared + hmg_massfn with the second stage of the contraction (the ordered sum over the
 * k' segments) folded into the mass-function launch: two launches instead of three, same sigma2 bits. */
int hmg_sigma2_massfn(hmg_ctx* ctx, int nz, int nm, int nq, const double* d_PT,
                      const double* d_kq, const double* d_wq, const double* d_R, double taylor_switch,
                      const hmg_massfn_params* h_par, const double* d_ms, const double* d_lnms,
                      const double* d_tinker_z, double* d_sigma2, double* d_nzm, double* d_bh);

/* ---- A5: concentration, virial radius, scale radius -----------------------------------
 * Replaces duffy_concentration / concentration / rvir (hmvec/hmvec.py:68-73,111-115,163-176).
 *   c = A (h m / 2e12)^alpha (1+z)^beta ;  rvir = (3 m / (4 pi delta[z] rho[z]))^(1/3) ;
 *   rs = rvir / c                                                                          */
int hmg_halo_structure(hmg_ctx* ctx, int nz, int nm, const double* d_ms, const double* d_zs,
                       const double* d_delta /*[nz]*/, const double* d_rho /*[nz]*/,
                       double duffy_A, double duffy_alpha, double duffy_beta, double h,
                       double* d_cs /*[nz][nm]*/, double* d_rvir /*[nz][nm]*/,
                       double* d_rs /*[nz][nm]*/);

/* hmg_halo_structure, the series rows of the analytic NFW kernel and hmg_mdelta_convert in ONE launch
 * (they are all one-thread-per-(z,m) stages that precede the profile kernels of a pass):
 *   d_nfw_series [nz][nm][HMG_NFW_SERIES_STRIDE] (or NULL): per-row coefficients of u_NFW's
 *     small-argument series and the row constants of its closed forms, to be handed to
 *     hmg_nfw_analytic, which otherwise computes them with a launch of its own;
 *   d_m2, d_r2 (both or NULL): the mass conversion of hmg_mdelta_convert with d_drho1, delta2, d_rho2.  */
#define HMG_NFW_SERIES_STRIDE 36
int hmg_halo_stage(hmg_ctx* ctx, int nz, int nm, const double* d_ms, const double* d_zs,
                   const double* d_delta /*[nz]*/, const double* d_rho /*[nz]*/,
                   double duffy_A, double duffy_alpha, double duffy_beta, double h,
                   double* d_cs, double* d_rvir, double* d_rs, double* d_nfw_series,
                   const double* d_drho1 /*[nz]*/, double delta2, const double* d_rho2 /*[nz]*/,
                   double* d_m2, double* d_r2);

/* Everything the constructor computes per (z,m) - hmg_sigma2_massfn and hmg_halo_stage (hmvec/hmvec.py:87-91,
 * 121-185 and :163-176, 225-227) - behind ONE launch after the sigma^2 contraction: the halo stage does not
 * depend on sigma^2, so its workgroups run beside the mass function's instead of waiting for a launch of
 * their own.  Same arithmetic, same results bit for bit as the two separate calls.                      */
typedef struct {
    const double *d_zs, *d_delta /*[nz]*/, *d_rho /*[nz]*/;
    double duffy_A, duffy_alpha, duffy_beta, h;
    double *d_cs, *d_rvir, *d_rs, *d_nfw_series /* or NULL */;
    const double* d_drho1 /*[nz]*/;
    double delta2;
    const double* d_rho2 /*[nz]*/;
    double *d_m2, *d_r2 /* both or NULL */;
} hmg_halo_stage_args;                 /* the arguments of hmg_halo_stage after d_ms, in its order */
int hmg_sigma2_massfn_halo(hmg_ctx* ctx, int nz, int nm, int nq, const double* d_PT,
                           const double* d_kq, const double* d_wq, const double* d_R, double taylor_switch,
                           const hmg_massfn_params* h_par, const double* d_ms, const double* d_lnms,
                           const double* d_tinker_z, double* d_sigma2, double* d_nzm, double* d_bh,
                           const hmg_halo_stage_args* h_halo);

/* ---- A7: mass-definition conversion -------------------------------------------------
 * Replaces mdelta_from_mdelta (hmvec/hmvec.py:748-798): the root in ln M2 of
 *   M1 F(c1) = M2 F(c2),  c2 = c1 ((M2/M1)(drho1/drho2))^(1/3),  F = 1/(ln(1+c)-c/(1+c)),
 * drho2[z] = delta2 * rho2[z].  Also returns r2 = (3 M2/(4 pi delta2 rho2))^(1/3)
 * (hmvec.py:225).                                                                       */
int hmg_mdelta_convert(hmg_ctx* ctx, int nz, int nm, const double* d_ms, const double* d_cs,
                       const double* d_drho1 /*[nz]*/, double delta2, const double* d_rho2 /*[nz]*/,
                       double* d_m2 /*[nz][nm]*/, double* d_r2 /*[nz][nm]*/);

/* ---- A6: analytic NFW u(k|m,z) --------------------------------------------------------
 * Replaces the Si/Ci branch of add_nfw_profile (hmvec/hmvec.py:346-353); Si/Ci follow
 * Cephes sici (scipy.special.sici).                                                     */
int hmg_nfw_analytic(hmg_ctx* ctx, int nz, int nm, int nk, const double* d_cs,
                     const double* d_rs, const double* d_zs, const double* d_ks,
                     const double* d_nfw_series /* from hmg_halo_stage for the SAME d_cs, or NULL */,
                     double* d_uk /*[nz][nm][nk]*/);

/* ---- A8/X1 row parameters of the generalised-NFW integrand ----------------------------
 * The three radial profiles of the path are one family
 *     f(x) = amp * (x/xc)^gamma * (1 + (x/xc)^alpha)^(-expo)
 *  NFW (hmvec.py:744): amp=1, xc=1, gamma=-1, alpha=1, expo=2
 *  Battaglia gas (hmvec.py:844-860): xc=1, alpha=alpha(m,z), expo=(beta+gamma)/alpha,
 *      amp=(Ob/Om) rho_c(z) rho0(m,z)
 *  Battaglia pressure (hmvec.py:906-927): xc=xc(m,z), alpha const, expo=beta(m,z),
 *      amp = eFrac (Ob/Om) 200 M G rho_c/(2 R200) P0(m,z)
 * with X(m,z) = A0 (m200c/1e14)^am (1+z)^az (hmvec.py:800-802).
 * fit[9] = {A0,am,az} x {rho0|P0, alpha|xc, beta}.  Outputs are [nz][nm].  The same launch
 * also emits the truncation radius cmax = rvir/rscale and rscale (hmvec.py:247-248,311-312)
 * and, for pressure, the y-conversion factor of hmvec.py:316.                              */
#define HMG_PROF_BATTAGLIA_GAS  1
#define HMG_PROF_BATTAGLIA_PRES 2
int hmg_profile_rowparams(hmg_ctx* ctx, int kind, int nz, int nm, const double* d_m200c,
                          const double* d_r200c, const double* d_rvir, const double* d_zs,
                          const double* d_rhocz /*[nz]*/, const double* d_hz /*[nz] H(z) in 1/Mpc, pressure only*/,
                          const double h_fit[9], double gamma, double alpha_const,
                          double amp_prefactor, double post_prefactor,
                          double* d_amp, double* d_xc, double* d_alpha, double* d_expo,
                          double* d_cmax /* rvir/rscale */, double* d_rscale /* R200c/2 (gas) or R200c (pressure) */,
                          double* d_post /* pressure: post_prefactor R200c^3 (1+z)^2/H(z); gas: may be NULL */);

/* hmg_mdelta_convert (with drho2 = delta2 * rhocz) + hmg_profile_rowparams in one launch; also
 * writes d_m200c / d_r200c.  Same results; one kernel boundary fewer per profile.           */
int hmg_profile_rows_from_mvir(hmg_ctx* ctx, int kind, int nz, int nm, const double* d_ms,
                               const double* d_cs, const double* d_rvir, const double* d_zs,
                               const double* d_drho1 /*[nz]*/, double delta2,
                               const double* d_rhocz /*[nz]*/, const double* d_hz /*[nz] or NULL*/,
                               const double h_fit[9], double gamma, double alpha_const,
                               double amp_prefactor, double post_prefactor,
                               double* d_m200c, double* d_r200c,
                               double* d_amp, double* d_xc, double* d_alpha, double* d_expo,
                               double* d_cmax, double* d_rscale, double* d_post);

/* ---- F1-F3: radial-profile sine transform + per-(z,m) k-interpolation ------------------
 * Replaces generic_profile_fft / fft_integral / _interp_loop (hmvec/fft.py:35-115),
 * bug-compatibly (step=(x[-1]-x[0])/N, 0-based DFT phase, left=u[first k>0], right=0,
 * strict x>cmax truncation).  Any of d_amp/d_xc/d_alpha/d_expo may be NULL meaning the
 * constant given in *_const.  d_xs [nxs] and d_kts [nxs/2+1] are the x grid
 * (linspace(0,xmax,nxs+1)[1:]) and the rfftfreq(nxs,fft_step)*2pi grid, built by the caller;
 * fft_step = (xs[-1]-xs[0])/nxs (hmvec/fft.py:45-47).  d_kts must be that uniform mode grid,
 * kts[j] = j * kts[1]: the in-LDS transform forms 1/kt_j as (1/j) / kt_1 and brackets the target
 * wavenumbers by division with the mode spacing.
 * out[z,m,k] *= d_post[z,m] if d_post != NULL (pressure prefactor, hmvec.py:316).
 *
 * Routes (chosen by the library from the radial grid and the rows' support; same results to <= 1e-12 in u, and each
 * within K 2^-52 S(k) |post| of the 40-digit discrete transform of the same float64 inputs, S the l1 scale of the row's
 * sum and K between 0.2 and 1.1 per route (3.9 for hmg_profile_fft_table, whose scale carries no integrand weights):
 * DESIGN.md section 30, tests/test_gpu_profile_rows.py):
 *   nxs = 1000, 2000, 4000, 5000      one (z,m) row per workgroup, packed-real FFT in LDS, compile-time plan;
 *   other even nxs <= 12288 (M = nxs/2 <= HMG_FUSED_MAX_M = 6144) whose half factors into 2, 3, 4, 5 with at most four
 *     butterflies per thread in every pass: the same with a run-time plan - for M > 2500 (HMG_FUSED_PREFER_M) only
 *     when the long-grid routes below do not apply (they are tried first there);
 *   longer grids - the ones the reference's own callers use: add_battaglia_profile(xmax=50, nxs=30000)
 *     (examples/lensing_baryons.py:27, bin/tests.py:308), numeric NFW nxs=40000 / xmax=200 (hmvec/params.py:59-60) -
 *     whose half is a multiple of a compiled sub-transform length LP >= the rows' support (profiles are cut at
 *     cmax << xmax): the long-grid kernels (R = nxs/2/LP pairs of length-LP transforms in LDS, or the chirp transform
 *     for rows that need few modes).  An EAGER call measures the support bound of its rows (one small kernel, a
 *     4-byte copy, one stream synchronisation) unless hmg_profile_support_epoch has tagged the arrays' contents;
 *     inside a captured step the bound on file for the same arrays is used (none on file: the one-row route if the
 *     length has one, else an error) and every row re-checks itself: a row beyond the bound is filled with NaN and
 *     the next synchronising call (hmg_sync, hmg_memcpy_d2h, hmg_event_synchronize) returns an error.  The tables of
 *     these routes do not depend on HMG_FUSED_MAX_M;
 *   long grids whose support does NOT prune but whose rows all need few modes (2 jn + 2 <= 1000..1250; the tSZ notebook's
 *     add_battaglia_pres_profile(xmax=2, nxs=30000)): the narrow-band kernel - nxs/2/LB transforms of length LB of the
 *     decimated row, one accumulator per needed mode; needs the hint arrays (ascending d_ks); the bound on the needed
 *     modes is measured and re-checked like the support bound;
 *   everything else (odd nxs, other prime factors, wide supports with many modes): integrand -> rocFFT R2C -> interpolation.
 * Environment switches for testing, read at hmg_ctx_create: HMG_FUSED_FFT=0 (rocFFT for everything), HMG_PRUNED_FFT=0,
 * HMG_CHIRP=0, HMG_BAND_FFT=0, HMG_PRUNED_LP_MIN, HMG_FUSED_MAX_M, HMG_FUSED_PREFER_M.                             */
int hmg_profile_fft(hmg_ctx* ctx, int nz, int nm, int nk, int nxs, double fft_step,
                    const double* d_xs, const double* d_kts,
                    const double* d_amp, const double* d_xc, const double* d_alpha,
                    const double* d_expo, double amp_const, double xc_const,
                    double alpha_const, double expo_const, double gamma,
                    const double* d_cmax /*[nz][nm]*/, const double* d_rss /*[nz][nm]*/,
                    const double* d_zs, const double* d_ks, int do_mass_norm,
                    const double* d_post /*[nz][nm] or NULL*/,
                    double* d_out /*[nz][nm][nk]*/,
                    int* d_nconst /*[nz][nm] or NULL*/, double* d_cconst /*[nz][nm] or NULL*/,
                    const double* d_logxs /*[nxs] from hmg_profile_fft_logx for the SAME d_xs, or NULL*/);
/* Tag of the CONTENTS of the d_cmax / d_rss / d_zs / d_ks arrays the following profile calls of this context will be
 * given (0, the default: no tag).  The long-grid routes size their launches from a bound on the rows' support and on
 * the modes they need; an untagged eager call measures that bound every time (a stream synchronisation).  With a
 * non-zero tag the bound measured by the first call with the same arrays, sizes and tag is reused - no host
 * synchronisation in later calls - on the caller's promise that equal tags mean equal contents.  A promise that
 * does not hold is caught, not computed through: every row re-checks itself, a row beyond the bound is filled with
 * NaN and the next synchronising call (hmg_sync, hmg_memcpy_d2h, hmg_event_synchronize) fails and drops the cached
 * bounds.  (The facade tags per model and mass grid: a model's concentrations and radii do not change.)          */
int hmg_profile_support_epoch(hmg_ctx* ctx, long long epoch);
/* ln xs[n]: the same for every (z,m) row, so a caller whose x grid does not change between passes
 * computes it once and hands it to hmg_profile_fft (one transcendental fewer per sample; without it
 * the kernel evaluates the logarithm itself, or builds the table per call when there are many rows). */
int hmg_profile_fft_logx(hmg_ctx* ctx, int nxs, const double* d_xs, double* d_logxs);
/* d_nconst / d_cconst (both or neither): constant-prefix hint of every output row for hmg_tracer -
 * the number of leading target wavenumbers below the row's first FFT mode and the value they all
 * receive.  With the hint arrays d_ks MUST be ascending (the caller's responsibility): the kernel finds the end of
 * that prefix by a search and fills it without loading or testing its wavenumbers; for a target grid in any
 * other order pass NULL for both.                                                                */

/* ---- deferred left fill of a hinted tensor (opt-in; off in a new context) ---------------------------------
 * 63 % of the Battaglia tensor at the headline shape is the constant prefix the hint arrays describe, and the
 * batched mass integrals (hmg_power_batch*, given the hints in their tracers) never load a k tile that lies in
 * it.  With deferral ON, a one-row-in-LDS transform that is given hint arrays leaves the whole
 * HMG_PREFIX_TILE-wide tiles of every row's prefix UNWRITTEN: elements [0, nconst[row] & ~(HMG_PREFIX_TILE-1))
 * keep whatever the buffer held; the rest of the row, d_nconst and d_cconst are written as always.  The context
 * remembers per tensor pointer that its prefix is pending - for eager calls at the call, for a captured step at
 * every replay - until the next filling call, a transform into the same buffer that writes it whole (deferral
 * off, no hints, the long-grid and rocFFT routes: they never defer), or the release of its block.
 * Every reader other than the batched mass integrals - the one-pair entry points, a copy to the host, the
 * caller's own kernels - must be preceded by the fill below; a filled tensor is bit-identical to the one a
 * transform without deferral writes.  HMG_PREFIX_TILE is a multiple of every k-tile width of the batched mass
 * integrals (asserted where they are compiled).
 *
 * Series deferral of the analytic NFW tensor.  The same switch covers the NFW rows of hmg_group_tensors: 61 % of
 * that tensor at the headline shape are whole tiles of a row's short-series band - the leading wavenumbers with
 * (1+c) k r_s (1+z) <= 0.8, a 5- or 8-term polynomial of the row's series coefficients.  With deferral ON and on the
 * tensor-group route (ascending d_ks) the rows leave elements [0, nser[row] & ~(HMG_PREFIX_TILE-1)) UNWRITTEN, nser[row] being the length of the band (an array the context
 * owns).  hmg_power_batch* finds the tensor in the context's books by its pointer and EVALUATES the k tiles that lie
 * in the band with the device function the rows use - the same bits, no load; tracers carry nothing new.  Every other
 * native reader fills first, on its own: hmg_power, hmg_power_2halo_terms, hmg_trispectrum_1h, hmg_bispectrum, hmg_response,
 * hmg_memcpy_d2h / _d2h_async / _d2d (source), hmg_fn2d / hmg_add / hmg_trapz_rows (inputs), and a batch that cannot
 * substitute (generic forms, the tensor not in slot 0).  The fill reads the row's c, r_s, z,
 * wavenumbers and series coefficients through the pointers the deferring launch was given: they must still hold what
 * that launch read.  hmg_memcpy_h2d / _h2d_async and hmg_memcpy_d2d INTO the tensor, a launch that writes it whole
 * (hmg_nfw_analytic, hmg_group_rows, hmg_group_tensors without deferral) and hmg_free drop the entry.  A reader
 * OUTSIDE the library (the caller's own kernel on the raw pointer) calls hmg_prefix_fill first, as for a hinted
 * tensor; hmg_prefix_pending reports the state.  hmg_nfw_analytic and hmg_group_rows never defer.              */
#define HMG_PREFIX_TILE 128
int hmg_prefix_deferral(hmg_ctx* ctx, int on);
/* Fill the pending prefix of the tensor at d_out on the current lane; nothing is enqueued when none is pending.
 * Inside a captured step the fill is recorded whenever the context has ever seen a deferred transform into d_out
 * (what a replay leaves pending is decided per replay, not at capture time).                                  */
int hmg_prefix_fill(hmg_ctx* ctx, double* d_out);
int hmg_prefix_pending(hmg_ctx* ctx, const double* d_out, int* h_pending);
/* The fill itself, for a caller that keeps its own books: d_cconst[row] into [0, d_nconst[row] & ~(HMG_PREFIX_TILE-1))
 * of each of the `rows` rows of nk doubles.                                                                    */
int hmg_prefix_fill_rows(hmg_ctx* ctx, double* d_out, const int* d_nconst, const double* d_cconst, int rows, int nk);

/* ---- H1-H3: HOD occupations ----------------------------------------------------------------
 * Replaces avg_Nc/avg_Ns/avg_NsNsm1/avg_NcNs, Mstellar_halo/Mhalo_stellar, get_ngal/get_bg
 * (hmvec/hmvec.py:634-731,462-466,936-957).  corr: 0 = "max", 1 = "min".                       */
typedef struct {
    double sig_log_mstellar, alphasat, Bsat, betasat, Bcut, betacut;
    int    corr;
} hmg_hod_params;
int hmg_hod(hmg_ctx* ctx, int nz, int nm, const hmg_hod_params* h_par, const double* d_zs,
            const double* d_ms, const double* d_log10mstar_thresh /*[nz]*/,
            const double* d_nzm, const double* d_bh, const double* d_wm /*[nm] trapz weights*/,
            double* d_Nc, double* d_Ns, double* d_NsNsm1, double* d_NcNs /*[nz][nm] each*/,
            double* d_ngal /*[nz]*/, double* d_bg /*[nz]*/);

/* ---- P1-P4: fused 1-halo + 2-halo mass integrals ---------------------------------------------
 * Replaces _get_matter/_get_hod/_get_hod_square/_get_pressure + get_power_1halo +
 * get_power_2halo (hmvec/hmvec.py:469-572) in ONE pass over the profile tensors:
 *   P1h[z,k] = trapz_m[n W_a W_b] (1-exp(-(k/kstar)^2))
 *   P2h[z,k] = Pzk (I_a + b_a - C_a)(I_b + b_b - C_b)
 * Either output pointer may be NULL.                                                          */
#define HMG_TRACER_MATTER   0
#define HMG_TRACER_HOD      1
#define HMG_TRACER_PRESSURE 2
typedef struct {
    int kind;                       /* HMG_TRACER_* */
    const double* d_prof;           /* matter: uk; pressure: pk; HOD: satellite uk   [nz][nm][nk] */
    const double* d_cprof;          /* HOD: central uk, or NULL meaning u_c == 1 */
    const double *d_Nc, *d_Ns, *d_NcNs, *d_NsNsm1, *d_ngal;   /* HOD only */
    const double* d_bias_override;  /* [nz] replaces b (b1_in/b2_in), or NULL */
    /* Optional constant-prefix hints for the two profile tensors (NULL = none): the first
     * nconst[z][m] entries of row (z,m) all equal cconst[z][m].  hmg_profile_fft can emit them
     * (np.interp's left fill, hmvec/fft.py:107: every target k below the first FFT mode gets the
     * same value - 63 % of a Battaglia tensor at Config 3).  hmg_power_batch then substitutes the
     * constant instead of reading those parts of the tensor; results are bit-identical.         */
    const int*    d_prof_nconst;   const double* d_prof_cconst;      /* [nz][nm] each */
    const int*    d_cprof_nconst;  const double* d_cprof_cconst;
} hmg_tracer;
int hmg_power(hmg_ctx* ctx, int nz, int nm, int nk, const hmg_tracer* h_a, const hmg_tracer* h_b,
              const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm,
              const double* d_ks, const double* d_Pzk, double rho_m0, double kstar,
              double* d_P1h /*[nz][nk] or NULL*/, double* d_P2h /*[nz][nk] or NULL*/);

/* The terms get_power_2halo(verbose=True) prints (hmvec/hmvec.py:566-571): the two 2-halo
 * integrals I_a(z,k), I_b(z,k) [nz][nk] and their k -> 0 consistency limits d_C12[z] = {C_a, C_b}. */
int hmg_power_2halo_terms(hmg_ctx* ctx, int nz, int nm, int nk, const hmg_tracer* h_a, const hmg_tracer* h_b,
                          const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm,
                          const double* d_ks, double rho_m0,
                          double* d_I1 /*[nz][nk]*/, double* d_I2 /*[nz][nk]*/, double* d_C12 /*[nz][2]*/);

/* Same integrals for SEVERAL spectra in one pass: ntr tracers (<= 4) over their distinct
 * profile tensors (<= 4), npairs (a,b) index pairs into h_tr.  Each distinct tensor is streamed
 * from HBM once for the whole batch instead of once per pair.  h_P1h[i] / h_P2h[i] are the
 * device outputs of pair i (either may be NULL).  The reference's first-name-only rule for
 * two DIFFERENT HOD (or two different pressure) names (hmvec.py:510-513) is not expressible
 * here: issue those pairs through hmg_power.  No bias overrides.                              */
int hmg_power_batch(hmg_ctx* ctx, int nz, int nm, int nk, int ntr, const hmg_tracer* h_tr,
                    int npairs, const int* h_pair_a, const int* h_pair_b,
                    const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm,
                    const double* d_ks, const double* d_Pzk, double rho_m0, double kstar,
                    double* const* h_P1h, double* const* h_P2h);

/* ---- grouped launches: independent stages of a pass as block ranges of ONE grid ---------------------
 * The reference runs its stages one numpy expression after another (hmvec/hmvec.py:127-131, 188-250,
 * 318-355, 357-460, 504-572); which of them do NOT depend on each other is a property of the model:
 *     sigma^2 contraction, halo stage (c, r_vir, r_s, M_200c)          need inputs only
 *     n(z,m), b(z,m)        <- sigma^2           HOD  <- n, b
 *     NFW u(k), Battaglia row parameters <- halo stage    profile FFT rows <- row parameters
 *     coefficient rows of the mass integrals <- n, b, HOD;   mass integrals <- those + the tensors
 * A kernel boundary costs ~2 us and every per-(z,m) stage is latency-bound, so on a thin z-slab (a rank
 * of an 8-GPU job: 4 redshifts) the small stages take a third of the step when each is its own launch.
 * The three entry points below put independent stages into one launch each: short latency-bound
 * workgroups first in the grid, the chip-filling ones behind them.  Every part is optional (NULL); a
 * part has the arguments of its stand-alone entry point and produces the same bits.  Per-z CHAIN =
 * HOD (or only its n_gal, b_g sums) -> coefficient rows, each link optional, one workgroup per redshift. */
typedef struct {   /* second stage of the contraction + n, b: hmg_sigma2_massfn's arguments after taylor_switch */
    const hmg_massfn_params* h_par;
    const double *d_ms, *d_lnms, *d_tinker_z;
    double *d_sigma2, *d_nzm, *d_bh;
} hmg_massfn_part;
#define HMG_HOD_ALL         0   /* occupation numbers and the n_gal, b_g sums (= hmg_hod) */
#define HMG_HOD_OCCUPATIONS 1   /* <Nc>, <Ns>, <Ns(Ns-1)>, <NcNs> only: they depend on inputs alone (z, m, threshold) */
#define HMG_HOD_SUMS        2   /* n_gal, b_g from stored occupations and n, b */
typedef struct {   /* hmg_hod's arguments + which half */
    int stage;
    const hmg_hod_params* h_par;
    const double *d_zs, *d_ms, *d_log10mstar_thresh, *d_nzm, *d_bh, *d_wm;
    double *d_Nc, *d_Ns, *d_NsNsm1, *d_NcNs, *d_ngal, *d_bg;
} hmg_hod_part;
typedef struct {   /* hmg_profile_rowparams's arguments */
    int kind;
    const double *d_m200c, *d_r200c, *d_rvir, *d_zs, *d_rhocz, *d_hz;
    double fit[9], gamma, alpha_const, amp_prefactor, post_prefactor;
    double *d_amp, *d_xc, *d_alpha, *d_expo, *d_cmax, *d_rscale, *d_post;
    /* ABI 8, optional (d_rowsc NULL: none): the OUTPUT-side scalars of every profile row, worked out here once per row by
     * the thread that has just computed the row's length scale instead of by one wavefront of every row workgroup of
     * hmg_profile_fft (hmvec/fft.py:96-107: k_out = kt / (r_s (1+z)), np.interp's left fill below kt_1 / (r_s (1+z))).
     * d_rowsc [nz*nm][HMG_ROWSC_STRIDE]: 1/(rscale (1+z)), k_lo = kt_1 that, k_hi = kt_M that, 1/k_lo, 1/kt_1, and - packed
     * in one double, high word first - the number of FFT modes the target grid can reach and the length of the left-fill
     * prefix.  Needs d_ks ASCENDING ([nk]), d_kts ([fft_m + 1]), fft_m = nxs/2 of the transform that will read it.       */
    const double *d_ks, *d_kts;
    int nk, fft_m;
    double* d_rowsc;
} hmg_rows_part;
#define HMG_ROWSC_STRIDE 8
typedef struct {   /* hmg_nfw_analytic's arguments (d_nfw_series is required here) */
    const double *d_cs, *d_rs, *d_zs, *d_ks, *d_nfw_series;
    double* d_uk;
} hmg_nfw_part;
typedef struct {   /* hmg_profile_fft's arguments after nk */
    int nxs;
    double fft_step;
    const double *d_xs, *d_kts, *d_amp, *d_xc, *d_alpha, *d_expo;
    double amp_const, xc_const, alpha_const, expo_const, gamma;
    const double *d_cmax, *d_rss, *d_zs, *d_ks;
    int do_mass_norm;
    const double* d_post;
    double* d_out;
    int* d_nconst;
    double* d_cconst;
    const double* d_logxs;
    const double* d_rowsc;   /* ABI 8, optional: the row scalars an hmg_rows_part with the same d_ks, d_kts, nxs/2 left (needs the hint arrays) */
} hmg_profile_fft_part;
typedef struct {   /* hmg_power_batch's arguments after nk */
    int ntr;
    const hmg_tracer* h_tr;
    int npairs;
    const int *h_pair_a, *h_pair_b;
    const double *d_nzm, *d_bh, *d_ms, *d_wm, *d_ks, *d_Pzk;
    double rho_m0, kstar;
    double* const* h_P1h;
    double* const* h_P2h;
} hmg_power_batch_desc;
/* front: first stage of the sigma^2 contraction (hmg_sigma2_prepared's arguments; the partial sums stay
 * in the context until a massfn part consumes them) beside the halo stage and, optionally, the occupation
 * numbers of an HOD (stage HMG_HOD_OCCUPATIONS) and the row parameters of a Battaglia profile - everything
 * of a pass that needs inputs only.                                                                       */
int hmg_sigma2_halo_front(hmg_ctx* ctx, int nz, int nm, int nq, const double* d_PT, const double* d_kq,
                          const double* d_wq, const double* d_R, double taylor_switch,
                          const double* d_ms, const hmg_halo_stage_args* h_halo,
                          const hmg_hod_part* h_hod_occupations /* or NULL */,
                          const hmg_rows_part* h_rows /* or NULL: Battaglia row parameters from the M_200c, R_200c,
                                                         r_vir this call's halo stage computes (same arrays) */);
/* rows group: n(z,m), b(z,m) in 62-mass tiles | per-z chain (an HOD; not together with a massfn part, whose
 * n, b it would need) | Battaglia row parameters | analytic NFW rows.  A massfn part needs the partial sums
 * of the last hmg_sigma2_halo_front on this context with the same nz, nm, nq.                           */
int hmg_group_rows(hmg_ctx* ctx, int nz, int nm, int nk, int nq, const hmg_massfn_part* h_massfn,
                   const hmg_hod_part* h_hod, const hmg_rows_part* h_rows, const hmg_nfw_part* h_nfw);
/* profile group: per-z chain (an HOD or its sums -> the coefficient rows of the batched mass integrals
 * h_prep describes) | the rows of one hmg_profile_fft (lengths its in-LDS transform takes; otherwise the
 * parts are issued one after the other).  After a call with h_prep, hmg_power_batch_run(...,
 * HMG_PB_PREPARED) with the SAME description runs the mass integrals without their preparation launch. */
int hmg_group_profile(hmg_ctx* ctx, int nz, int nm, int nk, const hmg_profile_fft_part* h_fft,
                      const hmg_hod_part* h_hod, const hmg_power_batch_desc* h_prep);
/* tensor group: everything between the front and the mass integrals as ONE launch - per-z chain (sigma^2 second stage +
 * n, b of h_massfn -> the sums of h_hod -> the coefficient rows h_prep describes; each link optional) | the rows of
 * h_fft | the analytic NFW rows of h_nfw.  What hmg_group_rows(massfn, nfw) followed by hmg_group_profile(fft, hod,
 * prep) compute, bit for bit, with one kernel boundary less: the chain's first link is done per redshift by the
 * chain's own workgroup instead of by mass tiles of an earlier launch.  Lengths whose transform shares no launch
 * (long grids, rocFFT route, no row scalars) run as separate launches behind the same call.  h_fft is required;
 * a massfn part needs the partial sums of the last hmg_sigma2_halo_front, as in hmg_group_rows.  (ABI 9)         */
int hmg_group_tensors(hmg_ctx* ctx, int nz, int nm, int nk, int nq, const hmg_massfn_part* h_massfn /* or NULL */,
                      const hmg_hod_part* h_hod /* or NULL */, const hmg_power_batch_desc* h_prep /* or NULL */,
                      const hmg_nfw_part* h_nfw /* or NULL */, const hmg_profile_fft_part* h_fft);
#define HMG_PB_PREPARED 1
int hmg_power_batch_run(hmg_ctx* ctx, int nz, int nm, int nk, const hmg_power_batch_desc* h_desc, int flags);

/* d_out[i] = d_a[i] + d_b[i]: HaloModel.get_power = get_power_1halo + get_power_2halo (hmvec/hmvec.py:500-502)
 * summed on the device, so that one (nz,nk) array crosses PCIe instead of two.                          */
int hmg_add(hmg_ctx* ctx, size_t n, const double* d_a, const double* d_b, double* d_out);

/* ---- N1: Limber projection ------------------------------------------------------------------
 * Replaces limber_integral (hmvec/cosmology.py:867-904): for every multipole,
 *   C_ell = sum_g wz[g] * pref[g] * P(z = gzs[g], k = (ell + 1/2)/chis[g]),
 * P bilinear in (z,k) on the (nz,nk) grid and clamped to it; pref = H W1 W2 / chi^2 built by
 * the caller; wz = trapezoid weights over gzs (a single 1 for a delta-function window).
 * nz == 1 does 1-D interpolation in k.                                                        */
int hmg_limber(hmg_ctx* ctx, int nells, const double* d_ells, int nz, int nk, const double* d_zs,
               const double* d_ks, const double* d_Pzk,
               const double* d_Pzk2 /* optional second (nz,nk) array added to d_Pzk on the fly
                                       (P_1h + P_2h without materialising the sum), or NULL */,
               int ngz, const double* d_gzs,
               const double* d_pref, const double* d_chis, const double* d_wz, double* d_out);

/* ---- module-level helpers of the path -------
 * The reference exports its building blocks as free functions (hmvec/__init__.py:1 star-import);
 * its own tests call them (bin/tests.py:11,27,268-295).  hmg_fn2d evaluates one of them over a
 * (rows, cols) grid: element (r,c) of input i is d_in[i][r*h_sr[i] + c*h_sc[i]], so full arrays
 * (sr=cols, sc=1), per-row (1,0), per-column (0,1) and scalar (0,0) operands broadcast as numpy
 * would.  h_par are host scalars.  One fp64 output [rows][cols].                                 */
#define HMG_FN_TINKER_BIAS    0  /* in nu; par delta                              tinker.py:26-40 */
#define HMG_FN_TINKER_FNU     1  /* in nu, z, table_z[nt], table_alpha[nt] (strides ignored for
                                    the two tables); par norm_consistency, alpha, nt  tinker.py:43-67 */
#define HMG_FN_MHALO_STELLAR  2  /* in z, log10mstellar                        hmvec.py:648-695 */
#define HMG_FN_HOD_NC         3  /* in log10mstar(m), log10mstar_thresh; par sigma  hmvec.py:698-703 */
#define HMG_FN_HOD_NS         4  /* in Nc, log10mhalo, Msat, Mcut; par alphasat   hmvec.py:708-716 */
#define HMG_FN_HOD_MFUNC      5  /* in log10mthresh; par Bamp, Bind                 hmvec.py:706 */
#define HMG_FN_HOD_NSNSM1     6  /* in Nc, Ns; par corr (0 max, 1 min)            hmvec.py:719-725 */
#define HMG_FN_HOD_NCNS       7  /* in Nc, Ns; par corr                           hmvec.py:727-731 */
#define HMG_FN_FCON           8  /* in c                                            hmvec.py:737 */
#define HMG_FN_RHO_NFW        9  /* in r, rhoscale, rs                            hmvec.py:744-746 */
#define HMG_FN_R_FROM_M      10  /* in M, rho, delta                              hmvec.py:627-628 */
#define HMG_FN_DUFFY         11  /* in m, z; par A, alpha, beta, h                 hmvec.py:68-73 */
#define HMG_FN_BATT_FIT      12  /* in m200c, z; par A0, alpha_m, alpha_z         hmvec.py:800-802 */
#define HMG_FN_RHO_GAS_X     13  /* in x, m200c, z, rhocritz; par omb, omm, gamma, fit[9]  :844-860 */
#define HMG_FN_RHO_GAS_R     14  /* in r, m200c, z, rhocritz; same par                    :819-842 */
#define HMG_FN_PE_X          15  /* in x, m200c, R200c, z, rhocritz; par omb, omm, alpha, gamma,
                                    fit[9], G_newt                                hmvec.py:906-927 */
#define HMG_FN_PE_R          16  /* in r, m200c, z, rhocritz; same par            hmvec.py:881-904 */
#define HMG_FN_NGAL_INTEGRAND 17 /* in nzm, Nc, Ns -> nzm*(Nc+Ns)                   hmvec.py:956 */
#define HMG_FN_A2Z           18  /* in a                                            hmvec.py:933 */
#define HMG_FN_MDELTA        19  /* in M1, c1, delta_rho1, delta_rho2 -> M2        hmvec.py:748-798 */
#define HMG_FN_BG_INTEGRAND  20  /* in nzm, Nc, Ns, bh -> nzm*(Nc+Ns)*bh            hmvec.py:464-466 */
#define HMG_FN_ST_FSIGMA     21  /* in sigma2; par st_A, st_a, st_p, deltac  (get_fsigmaz, ST)  hmvec.py:136-141 */
#define HMG_FN_TINKER_FSIGMA 22  /* in sigma2, z, table_z, table_alpha; par as TINKER_FNU + deltac:
                                    nu f_nu(nu, z) with nu = deltac/sigma   (get_fsigmaz)      hmvec.py:142-145 */
#define HMG_FN_WKR           23  /* in k, R; par taylor_switch: Fourier top-hat W(kR)    cosmology.py:30-38 */
#define HMG_FN_LINCOMB3      24  /* in X0, X1, X2; par a, b, c -> a X0 + b X1 + c X2
                                    (total_matter_power_spectrum etc.)                 cosmology.py:599-658 */
#define HMG_FN_MHALO_STELLAR_CORE 25 /* in log10mstellar, a; par Mstar00, Mstara, M1, M1a, beta0, beta_a, gamma0,
                                       gamma_a, delta0, delta_a                         hmvec.py:648-657 */
#define HMG_FN_BRUTE_INTEGRAND 26 /* in r, rho, k -> 4 pi r sin(r k) rho / k  (uk_brute_force)           fft.py:22-33 */
#define HMG_FN_COUNT         27
#define HMG_FN_MAXIN   6
#define HMG_FN_MAXPAR 16
int hmg_fn2d(hmg_ctx* ctx, int op, int rows, int cols, int nin, const double* const* h_d_in,
             const int* h_sr, const int* h_sc, const double* h_par, int npar, double* d_out);

/* Mstellar_halo (hmvec/hmvec.py:634-646): per-redshift inverse of the SHMR through the
 * reference's 4000-point table linspace(-18,18,4000) and np.interp (clamped ends).
 * d_log10mhalo [nm] is shared by every z, as in the reference (it reads row 0).  -> [nz][nm]    */
int hmg_mstellar_halo(hmg_ctx* ctx, int nz, int nm, const double* d_zs, const double* d_log10mhalo,
                      double* d_out);

/* np.trapz(y, x, axis=-1) for y [rows][cols], x [cols] (ngal_from_mthresh hmvec.py:957, the
 * mass normalisation of uk_fft fft.py:15).  -> [rows]                                           */
int hmg_trapz_rows(hmg_ctx* ctx, int rows, int cols, const double* d_y, const double* d_x, double* d_out);

/* fft_integral (hmvec/fft.py:35-51): uk_j = -Im(rfft(x*y))_j * step, step = (x[n-1]-x[0])/n, for
 * every row of y [rows][n]; d_uk [rows][n/2+1].  The wavenumbers 2*pi*rfftfreq(n, step) are a
 * host one-liner and are left to the caller.                                                    */
int hmg_sine_transform(hmg_ctx* ctx, int rows, int n, const double* d_x, const double* d_y, double* d_uk);

/* generic_profile_fft (hmvec/fft.py:56-94) for a TABULATED integrand: d_rho is rho(x) on
 * xs = linspace(0,xmax,nxs+1)[1:], either one row shared by all (z,m) (rho_rows == 1) or one row
 * per (z,m) (rho_rows == nz*nm) - the two shapes the reference accepts (fft.py:75-78).  Truncation
 * |x| > cmax, trapz mass norm, sine transform, k scaling and interpolation as hmg_profile_fft.  */
int hmg_profile_fft_table(hmg_ctx* ctx, int nz, int nm, int nk, int nxs, double fft_step,
                          const double* d_xs, const double* d_kts, const double* d_rho, int rho_rows,
                          const double* d_cmax, const double* d_rss, const double* d_zs,
                          const double* d_ks, int do_mass_norm, double* d_out);

/* ---- cluster-lensing profiles (hmvec/hmvec.py:574-625; DESIGN.md sections 10 and 12) ----------------------------
 * Per-halo inputs have n entries: scale radius r_s [Mpc], delta_c and rho_crit(z) [Msun/Mpc^3].  d_rbins holds the
 * projected radii [Mpc]: (n, nr) when rbins_per_halo != 0, else one row of nr shared by every halo.  d_out is (n, nr)
 * in Msun/Mpc^2.  Radii, r_s and offsets must be positive; the Python layer checks values, these check shapes.
 * hmg_lensing_sigma_nfw: Sigma of the centred NFW profile (Wright & Brainerd 2000, eq. 11, with a series around
 *   x = 1).
 * hmg_lensing_sigma_nfw_off: the same averaged over Rayleigh-distributed centre offsets of width d_offsets[h] [Mpc]
 *   (2-D quadrature, one wavefront per output, bit-identical on repeat).  The first call on a device uploads its node
 *   table and so cannot be inside a captured step.
 * hmg_lensing_delta_sigma_nfw[_off]: same arguments and checks; store the excess surface density
 *   Delta Sigma(R) = Sigmabar(<R) - Sigma(R) (eqs. 13-15, with a series around x = 1 and a cancellation-free form at
 *   small x; miscentred: Sigma_off and the Rayleigh average of the centred profile's mass in an offset disc, from the
 *   same outer nodes and a second node table).                                                                     */
int hmg_lensing_sigma_nfw(hmg_ctx* ctx, int n, int nr, int rbins_per_halo, const double* d_rs, const double* d_delta_c,
                          const double* d_rho_crit, const double* d_rbins, double* d_out);
int hmg_lensing_sigma_nfw_off(hmg_ctx* ctx, int n, int nr, int rbins_per_halo, const double* d_rs,
                              const double* d_delta_c, const double* d_rho_crit, const double* d_rbins,
                              const double* d_offsets, double* d_out);
int hmg_lensing_delta_sigma_nfw(hmg_ctx* ctx, int n, int nr, int rbins_per_halo, const double* d_rs,
                                const double* d_delta_c, const double* d_rho_crit, const double* d_rbins,
                                double* d_out);
int hmg_lensing_delta_sigma_nfw_off(hmg_ctx* ctx, int n, int nr, int rbins_per_halo, const double* d_rs,
                                    const double* d_delta_c, const double* d_rho_crit, const double* d_rbins,
                                    const double* d_offsets, double* d_out);
/* Two-halo convergence, d_out (nz, ntheta, nM):
 *   b(z, M) pre(z) trapz_l[ P(z,k) J0(l theta) l / 2 pi ],  l = k chi(z) with lmin < l < lmax (strict, grid order),
 * pre(z) = rho_m(z) / (1+z)^3 / Sigma_crit(z) / D_A(z)^2 (nz), d_ks (nk) increasing, d_Pzk (nz, nk), d_thetas [rad]
 * (ntheta), b(z, M) the linear interpolation of d_bh (nz, nm) on d_ms (nm >= 2, increasing) at d_Ms (nM).
 * hmg_lensing_gamma_t_2h: same arguments and checks; J2(l theta) in place of J0 (Oguri & Takada 2011): the two-halo
 *   tangential shear, or with pre(z) without its 1/Sigma_crit the two-halo Delta Sigma [Msun/Mpc^2].               */
int hmg_lensing_kappa_2h(hmg_ctx* ctx, int nz, int nk, int ntheta, int nm, int nM, const double* d_ks,
                         const double* d_chi, const double* d_pre, const double* d_Pzk, const double* d_thetas,
                         double lmin, double lmax, const double* d_ms, const double* d_bh, const double* d_Ms,
                         double* d_out);
int hmg_lensing_gamma_t_2h(hmg_ctx* ctx, int nz, int nk, int ntheta, int nm, int nM, const double* d_ks,
                           const double* d_chi, const double* d_pre, const double* d_Pzk, const double* d_thetas,
                           double lmin, double lmax, const double* d_ms, const double* d_bh, const double* d_Ms,
                           double* d_out);

/* ---- kSZ forecasts (hmvec/ksz.py) ---------------------------------------------------------
 * hmg_ksz_pqperp: the Ma-Fry P_q_perp table d_out (nk, nz) for nz redshifts,
 *   out[k, z] = adotf[z]^2 (2 pi)^-2 trapz_mu trapz_k' nan_to_num(k'^2 k (k - 2k'mu)(1 - mu^2)
 *                                               / (k'^2 (k'^2 + k^2 - 2 k k' mu)) Pmm[z, k'] Pee[z, |k - k'|]),
 *   d_ks (nk) ascending (any spacing), d_mus (nmu <= 4096), d_Pee / d_Pmm (nz, nk) paired with d_ks, Pee linear in k
 *   with 0 outside [ks[0], ks[nk-1]], d_adotf (nz).                                                              */
int hmg_ksz_pqperp(hmg_ctx* ctx, int nz, int nk, int nmu, const double* d_ks, const double* d_mus,
                   const double* d_Pee, const double* d_Pmm, const double* d_adotf, double* d_out);
/* hmg_ksz_nvv: the kSZ reconstruction noise d_out (nz, nmu, nkL),
 *   Nvv = mu^-2 2 pi chi[z]^2 / F[z]^2 / trapz_kS _sanitize(kS (W Pge)^2 / ((W^2 Pgg + ngg[z]) C(chi[z] kS))),
 *   C(l) = d_cls[int(l)] for l <= ncl - 1 (0 below l = 2), inf above.  d_sig / d_H (nz) non-NULL: photo-z,
 *   W = exp(-sig^2 (mu kL)^2 / 2 / H^2), else W = 1.  d_Pge / d_Pgg / d_Pph are (nz, nkS) when rows == 0, or
 *   (nz, nmu, nkL, nkS) when rows == 1 (no photo-z then); d_Pph non-NULL: the robust term (integrand times
 *   Pph / (W^2 Pgg + ngg), sanitized).  *d_bad (one int on the device) is set to 1 when any output is non-finite. */
int hmg_ksz_nvv(hmg_ctx* ctx, int nz, int nmu, int nkL, int nkS, int ncl, int rows, const double* d_mus,
                const double* d_kLs, const double* d_kSs, const double* d_cls, const double* d_chi, const double* d_F,
                const double* d_sig, const double* d_H, const double* d_ngg, const double* d_Pge,
                const double* d_Pgg, const double* d_Pph, double* d_out, int* d_bad);
/* hmg_ksz_limber_cl: C_ell^kSZ d_out (nell) = trapz over the nchi nodes d_chi[l, :] (redshifts d_zn[l, :]) of
 *   P(z, ell / chi) / (chi^2 / (1+z)^4) * 0.5 * c2 * T2    (squeezed == 0, Ma-Fry)
 *   P(z, ell / chi) / chi^2 * (1+z)^4 * c2 * T2            (squeezed == 1)
 * with P bilinear and edge-clamped on the table d_P (nk, nz) over d_zs (nz >= 2) and d_ks (nk >= 2), ascending. */
int hmg_ksz_limber_cl(hmg_ctx* ctx, int nell, int nchi, int nz, int nk, const double* d_ells, const double* d_chi,
                      const double* d_zn, const double* d_zs, const double* d_ks, const double* d_P, int squeezed,
                      double c2, double T2, double* d_out);

/* ---- correlation function of tabulated spectra -------------------------------------------
 * hmg_xi_transform: d_out (rows, nr), out[row, j] = xi(rs[j]) of the row d_P[row, :],
 *   xi(r) = 1/(2 pi^2 r) int f~(k) sin(k r) dk,
 * f~ the piecewise-linear interpolant of f_i = ks[i] P[row, i] on [ks[0], ks[nk-1]] and zero outside, the integral
 * exact panel by panel (no quadrature in k r).  d_ks (nk >= 2) positive and strictly increasing, d_P (rows, nk) finite,
 * d_rs (nr) positive, shared by all rows; the Python layer checks values, this checks shapes.  fp64, no atomics:
 * bit-identical on repeat, and a row's results do not depend on the other rows or radii of the launch.            */
int hmg_xi_transform(hmg_ctx* ctx, int rows, int nk, int nr, const double* d_ks, const double* d_P,
                     const double* d_rs, double* d_out);

/* ---- Hankel transforms of tabulated spectra: w_p, Sigma, Delta Sigma ----------------------
 * hmg_hankel_transform: d_w0 and d_w2 (rows, nr), w0[row, j] = W_0(rs[j]) and w2[row, j] = W_2(rs[j]) of d_P[row, :],
 *   W_n(R) = 1/(2 pi) int k P~(k) J_n(k R) dk,   n = 0, 2,
 * P~ the interpolant of P that is linear in k^2 on each panel of [ks[0], ks[nk-1]] and zero outside, the integrals
 * exact panel by panel.  Either output pointer may be NULL (that order is not computed), not both.  Arguments as for
 * hmg_xi_transform; fp64, no atomics: bit-identical on repeat, a row's results do not depend on the other rows or radii
 * of the launch, and an output does not depend on whether the other one was asked for.                             */
int hmg_hankel_transform(hmg_ctx* ctx, int rows, int nk, int nr, const double* d_ks, const double* d_P,
                         const double* d_rs, double* d_w0, double* d_w2);

/* ---- angular correlation functions of tabulated spectra: w(theta), gamma_t, xi+- ----------
 * hmg_angular_transform: d_w0, d_w2 and d_w4 (n * nz, nt), wN[row, j] = W_N(R) of d_P[row, :] at the radius
 *   R = fl(chis[row % nz] * thetas[j])    (one rounding),     W_N(R) = 1/(2 pi) int k P~(k) J_N(k R) dk,   N = 0, 2, 4,
 * P~ as for hmg_hankel_transform, the integrals exact panel by panel.  d_P (n * nz, nk): n blocks of nz rows, row z of
 * every block at the distance d_chis[z] (nz, positive); d_thetas (nt) positive, in radians.  Any output pointer may be
 * NULL (that order is not computed), not all three.  W_0 and W_2 are bit for bit what hmg_hankel_transform gives at
 * the radius R: both entry points launch one kernel, with the rule for R as a template argument.  fp64, no atomics:
 * bit-identical on repeat, a result depends on nk, ks, its row and its R alone, and an output does not depend on which
 * others were asked for.
 * hmg_angular_zsum: d_out (n, nw, nt), out[i, w, j] = sum_z zw[w, z] W[i * nz + z, j], d_zw (nw, nz), d_w (n * nz, nt):
 * one fused multiply-add chain over z in index order from 0.0 per output (a single z of weight 1.0 returns W's bits);
 * no atomics, no dependence on the launch shape.  d_out must not overlap d_w.                                       */
int hmg_angular_transform(hmg_ctx* ctx, int n, int nz, int nk, int nt, const double* d_ks, const double* d_P,
                          const double* d_chis, const double* d_thetas, double* d_w0, double* d_w2, double* d_w4);
int hmg_angular_zsum(hmg_ctx* ctx, int n, int nz, int nt, int nw, const double* d_zw, const double* d_w,
                     double* d_out);

/* ---- redshift-space correlation multipoles of tabulated multipole spectra -------------------
 * hmg_xi_multipoles: d_xi0, d_xi2 and d_xi4 (rows, ns), xiL[row, j] = xi_L(ss[j]) of the row of P_L,
 *   xi_L(s) = i^L / (2 pi^2) int k f~(k) j_L(k s) dk,   L = 0, 2, 4   (i^L = +1, -1, +1),
 * f~ the piecewise-linear interpolant of f_i = ks[i] P_L[i] on [ks[0], ks[nk-1]] and zero outside (hmg_xi_transform's),
 * the integral exact panel by panel.  Each order reads its own rows, element i of row r at
 * d_PL[r * row_stride + i * node_stride] (node_stride >= 1, row_stride >= (nk - 1) * node_stride + 1): contiguous rows
 * have (nk, 1); the (2, nz, n, 3) block of hmg_rsd_multipoles is read in place with (3 n, 3) and the bases d_out,
 * d_out + 1, d_out + 2.  An order is computed when its output pointer is non-NULL - its input pointer must then be
 * non-NULL too - and at least one is.  d_ks (nk >= 2) positive and strictly increasing, d_ss (ns) positive, shared by
 * all rows; the Python layer checks values, this checks shapes and strides.  xi_0 is bit for bit hmg_xi_transform of
 * the same row at r = s: that entry point launches this kernel with order 0 alone and the strides (nk, 1).  fp64, no
 * atomics: bit-identical on repeat, a result depends on nk, ks, its row and its s alone, not on which other outputs
 * were asked for nor on the strides.                                                                               */
int hmg_xi_multipoles(hmg_ctx* ctx, int rows, int nk, int ns, const double* d_ks, const double* d_P0,
                      const double* d_P2, const double* d_P4, long long row_stride, long long node_stride,
                      const double* d_ss, double* d_xi0, double* d_xi2, double* d_xi4);

/* ---- covariance of angular correlation functions -------------------------------------------
 * Flat sky, section 22's J_mu convention; mu = 0, 2, 4 is named by its index o = mu / 2.  For the annulus [a, b],
 *   K_mu(l; a, b) = 2 / ((b^2 - a^2) l^2) [F_mu(l b) - F_mu(l a)],
 *   F_0(x) = x J1(x),   F_2(x) = -x J1(x) - 2 J0(x),   F_4(x) = (x - 24/x) J1(x) + 8 J0(x),
 * the bin average of J_mu(l theta).  Spectra: d_C (nf, nf, nn), symmetric in the fields (the entry with f <= g is the
 * one read), at the nodes d_nodes (nn >= 2, strictly increasing, >= 1); C(l) is linear in l between nodes; d_noise (nf)
 * white noise levels >= 0.  The multipoles are the integers L = l0 .. l0 + nl - 1, which the caller keeps inside
 * [nodes[0], nodes[nn-1]].  Multipoles per partial sum and bins per workgroup tile:                               */
#define HMG_ANGCOV_CHUNK 1024
#define HMG_ANGCOV_TILE 32
/* hmg_angcov_weights: d_k0, d_k2, d_k4 (nl, nt), kN[l, i] = K_N(ells[l]; edges[i], edges[i+1]); d_ells (nl) positive,
 *   d_edges (nt + 1) positive and strictly increasing, in radians.  Any output may be NULL, not all three.  J0 and J1
 *   are evaluated once per (l, edge); a value depends on its l and its two edges alone.
 * hmg_angcov_gaussian: d_cov (np, nt, np, nt).  h_probes (np, 3) holds (f, g, o) per probe and d_probes the same ints on
 *   the device; with P = (a, b, mu), Q = (c, d, nu), C^^fg = C^fg + delta_fg N_f and area = 4 pi fsky,
 *     cov[P,i,Q,j] = 1/(2 pi area) sum_{l in L} l K_mu(l; i) K_nu(l; j) [C^^ac C^^bd + C^^ad C^^bc - NN](l)
 *                  + delta_ij delta_mu,nu (delta_ac delta_bd + delta_ad delta_bc) N_a N_b / (area pi (b_i^2 - a_i^2)),
 *   NN = (delta_ac delta_bd + delta_ad delta_bc) N_a N_b: the noise x noise product, a delta function in theta whose l
 *   sum does not converge, is left out of the sum and added in closed form, and dropped for mu != nu.  d_k0 / d_k2 /
 *   d_k4 are hmg_angcov_weights' outputs on L and d_edges (an order no probe names may be NULL); d_work holds
 *   work_words >= np (np + 1) / 2 * ceil(nl / HMG_ANGCOV_CHUNK) * nt^2 doubles.  The sum runs per pair P <= Q over
 *   chunks of HMG_ANGCOV_CHUNK multipoles counted from l0, each in l order from 0.0, and the chunks' sums are added in
 *   chunk order; Q < P is the transpose.  The Python layer checks values; this checks shapes, the probes' fields and
 *   orders and the size of the work buffer.
 * hmg_angcov_node_weights: d_r (nt, nn), or (nn, nt) if by_node, r[i, n] = scale * sum_{l in L} l K(l; i) h_n(l), h_n
 *   the hat function of node n and d_k (nl, nt) one order's weights on L; the same chunks and order of summation.
 * fp64, no atomics: bit-identical on repeat; an element of d_cov depends on its two probes, its two bins, the spectra
 * and L alone - not on the other probes or bins of the call, not on the order the probes or a probe's fields are
 * given in - and cov[P,i,Q,j] and cov[Q,j,P,i] are the same bits.                                                  */
int hmg_angcov_weights(hmg_ctx* ctx, int nl, int nt, const double* d_ells, const double* d_edges, double* d_k0,
                       double* d_k2, double* d_k4);
int hmg_angcov_gaussian(hmg_ctx* ctx, int nf, int nn, const double* d_nodes, const double* d_C, const double* d_noise,
                        int l0, int nl, int nt, const double* d_edges, int np, const int* h_probes, const int* d_probes,
                        double area, const double* d_k0, const double* d_k2, const double* d_k4, size_t work_words,
                        double* d_work, double* d_cov);
int hmg_angcov_node_weights(hmg_ctx* ctx, int nn, const double* d_nodes, int l0, int nl, int nt, const double* d_k,
                            double scale, int by_node, double* d_r);

/* ---- curved-sky angular correlation functions and their covariance -----------------------
 * The four kinds 0 .. 3 = w, gammat, xip, xim are the Wigner functions d^l = P_l, d^l_{0,2}, d^l_{2,2}, d^l_{2,-2} of
 * theta; xi_kind^{ab}(theta) = sum_l (2l + 1)/(4 pi) C_l^{ab} d_kind^l(theta).  For the annulus [a, b], 0 < a < b <= pi,
 *   K_kind(l; a, b) = [G_kind(l; b) - G_kind(l; a)] / (cos a - cos b),   G_kind(l; theta) = int_0^theta sin d_kind^l,
 * and a spin-2 kind (gammat, xip, xim) is exactly 0 below l = 2.  Spectra, nodes, noise levels and L = l0 .. l0 + nl - 1
 * are hmg_angcov_gaussian's.  d_cosdiff (nt) holds cos a_i - cos b_i of the bins, formed as 2 sin((a+b)/2) sin((b-a)/2)
 * by the caller: the weights and the noise term divide by the same numbers.
 * hmg_curvedsky_weights: d_kw, d_kg, d_kp, d_km (nl, nt), k[l - l0, i] = K_kind(l; edges[i], edges[i+1]); d_edges
 *   (nt + 1) in (0, pi], strictly increasing.  Any output may be NULL, not all four.  One thread per edge walks the
 *   three-term recurrences from l = 0; a value depends on its l and its two edges alone.
 * hmg_curvedsky_gaussian: d_cov (np, nt, np, nt); h_probes / d_probes (np, 3) hold (f, g, kind).  With area = 4 pi fsky,
 *     cov[P,i,Q,j] = 1/(4 pi area) sum_{l in L} (2l + 1) K_kind(l; i) K_kind'(l; j) [C^^ac C^^bd + C^^ad C^^bc - NN](l)
 *                  + delta_ij delta_kind,kind' (delta_ac delta_bd + delta_ad delta_bc) N_a N_b / (area 2 pi cosdiff[i]):
 *   hmg_angcov_gaussian's sum with the measure l + 1/2, the same kernels, chunks, order of summation, work buffer
 *   (work_words >= np (np + 1) / 2 * ceil(nl / HMG_ANGCOV_CHUNK) * nt^2) and bit-identities.  A kind no probe names may
 *   have a NULL weight pointer.
 * hmg_curvedsky_node_weights: hmg_angcov_node_weights with the measure l + 1/2,
 *   r[i, n] = scale * sum_{l in L} (l + 1/2) K(l; i) h_n(l).
 * hmg_curvedsky_scale_spectra: d_C (nf, nf, nn) in place, C[f, g, n] *= f(nodes[n])^(number of spin-2 fields among f
 *   and g), f(l) = sqrt((l + 2)(l - 1) / (l (l + 1))) (f^2 is formed as the ratio, without the root): convergence
 *   spectra to E-mode spectra.  h_spins / d_spins (nf) hold 0 or 2 per field, on the host and on the device.
 * This checks shapes, kinds, spins, l0 >= 1 and the size of the work buffer; the Python layer checks values.  fp64, no
 * atomics, bit-identical on repeat.  The largest multipole hmg_curvedsky_weights walks to (every workgroup steps its
 * recurrence from l = 0: 2^24 steps are a few tenths of a second):                                                  */
#define HMG_CURVEDSKY_LMAX 16777216
int hmg_curvedsky_weights(hmg_ctx* ctx, int l0, int nl, int nt, const double* d_edges, const double* d_cosdiff,
                          double* d_kw, double* d_kg, double* d_kp, double* d_km);
int hmg_curvedsky_gaussian(hmg_ctx* ctx, int nf, int nn, const double* d_nodes, const double* d_C, const double* d_noise,
                           int l0, int nl, int nt, const double* d_cosdiff, int np, const int* h_probes,
                           const int* d_probes, double area, const double* d_kw, const double* d_kg, const double* d_kp,
                           const double* d_km, size_t work_words, double* d_work, double* d_cov);
int hmg_curvedsky_node_weights(hmg_ctx* ctx, int nn, const double* d_nodes, int l0, int nl, int nt, const double* d_k,
                               double scale, int by_node, double* d_r);
int hmg_curvedsky_scale_spectra(hmg_ctx* ctx, int nf, int nn, const double* d_nodes, const int* h_spins,
                                const int* d_spins, double* d_C);

/* ---- non-Limber angular power spectra of separable sources -----------------------------------
 * A spectrum that is separable between two lines of sight, P(z, z', k) = S_a(z, k) S_b(z', k) - the two-halo term
 * P_lin L_a L_b is, with S = L sqrt(P_lin) - projects exactly through one transfer function per field:
 *   T_l^f(kq_i) = sum_g src[f, g, i] j_l(kq_i chi_g),       src = (weights of the chi rule) x (window) x S_f(z_g, kq_i),
 *   C_l^{ab} = (2/pi) sum_i wk_i kq_i^2 T_l^a(kq_i) T_l^b(kq_i),        l = 0 .. lmax.
 * hmg_sph_bessel: d_out (lmax + 1, nx), out[l, n] = j_l(xs[n]) by the walk of hmvec_amd/csrc/sphbessel.hpp: upwards for
 *   x >= lmax, Miller's downward recurrence from a start order that depends on lmax alone otherwise; a value below the
 *   fp64 range is 0, never NaN.  A value depends on its x and on lmax (through the branch and the start order).
 * hmg_nonlimber_transfer: d_out (F, lmax + 1, nkq) = T of d_src (F, ngz, nkq).  1 <= F <= HMG_NONLIMBER_FMAX per launch:
 *   the walk at a point (kq_i, chi_g) runs once for all fields.  One workgroup of HMG_NONLIMBER_THREADS lanes per k node
 *   walks the chi nodes in chunks of its width, orders in tiles of HMG_NONLIMBER_TILE through LDS; the sum over g has a
 *   fixed order.
 * hmg_nonlimber_cl: d_out (np, lmax + 1) = C_l of the pairs h_pairs / d_pairs (np, 2) of fields of d_T (F, lmax + 1, nkq).
 * Contract: fp64, no atomics, every sum in a fixed order, bit-identical on repeat.  An element of T depends on its
 * field's source column, its k node, the chi nodes and lmax alone - not on the other fields or the other k nodes of the
 * call; it DOES depend on lmax (the branch x >= lmax and the start order): T_l of a call to lmax + 2 is not bit for bit
 * T_l of a call to lmax.  C[P] does not depend on the other pairs, and C[(a, b)] and C[(b, a)] are the same bits.  This
 * checks shapes and field indices; the Python layer checks values (positive increasing nodes, kq chi >= 1e-100).      */
#define HMG_NONLIMBER_FMAX 16
#define HMG_NONLIMBER_THREADS 256
#define HMG_NONLIMBER_TILE 16
#define HMG_NONLIMBER_LMAX 16384
int hmg_sph_bessel(hmg_ctx* ctx, int lmax, int nx, const double* d_xs, double* d_out);
int hmg_nonlimber_transfer(hmg_ctx* ctx, int F, int ngz, int nkq, int lmax, const double* d_kq, const double* d_chis,
                           const double* d_src, double* d_out);
int hmg_nonlimber_cl(hmg_ctx* ctx, int F, int nkq, int lmax, int np, const int* h_pairs, const int* d_pairs,
                     const double* d_kq, const double* d_wk, const double* d_T, double* d_out);

/* ---- 1-halo trispectrum of two spectra -----------------------------------------------------
 * hmg_trispectrum_1h: d_T (nz, n, n),
 *   T[z,i,j] = sum_m wm[m] nzm[z,m] s_ab[z,m,i] s_cd[z,m,j],
 *   s_xy[z,m,i] = scale[z,i] ((1 - frac[z,i]) S_xy(z, m, k_idx[z,i]) + frac[z,i] S_xy(z, m, k_{idx[z,i]+1})),
 * (scale does not depend on m: the sum is taken without it and multiplied by scale[z,i] scale[z,j] as one factor),
 * S_xy the square term hmg_power integrates for the pair (x, y), with the reference's first-name-only rules for two HOD
 * and two pressure names (hmvec/hmvec.py:510-523).  Node idx + 1 is not read where frac == 0, so idx = nk-1 with
 * frac = 0 is legal.  d_Tz (n, n) = sum_z zweights[z] T[z], z in order, needs d_zweights; either output may be NULL,
 * not both (d_T NULL: the per-z matrices live in a temporary block).  n >= 1.  The tables are checked on the device
 * before any tensor is read through them - an idx outside 0 .. nk-1, a frac outside [0, 1], idx == nk-1 with
 * frac != 0 are errors - and the host waits for that answer: the call synchronises the current stream once and cannot be
 * part of a captured step.  Tracers as for hmg_power (hints and bias overrides are not read).  fp64 on the vector
 * units, every workgroup walks the whole mass axis in order, no atomics: bit-identical on repeat, an element depends
 * only on its own (z, i, j) sample entries, and T^{ab,cd}[z,i,j] has the bits of T^{cd,ab}[z,j,i].                  */
int hmg_trispectrum_1h(hmg_ctx* ctx, int nz, int nm, int nk, int n,
                       const hmg_tracer* h_a, const hmg_tracer* h_b, const hmg_tracer* h_c, const hmg_tracer* h_d,
                       const double* d_nzm, const double* d_ms, const double* d_wm, double rho_m0,
                       const int* d_idx /*[nz][n]*/, const double* d_frac, const double* d_scale,
                       const double* d_zweights /*[nz] or NULL*/,
                       double* d_T /*[nz][n][n] or NULL*/, double* d_Tz /*[n][n] or NULL*/);

/* ---- halo-model bispectrum of three tracers, 1h + 2h + 3h ------------------------------------
 * hmg_bispectrum: d_B (3, nz, nt) = (B1h, B2h, B3h) of the legs (a, b, c) at nt triangles tri[t] = (s1, s2, s3) of the n
 * samples per redshift (tables as for hmg_trispectrum_1h; leg a sits at s1, b at s2, c at s3; n <= 256, nt <= 2^20):
 *   B1h[z,t] = sigma D1 D2 D3 sum_m wm nzm w_a(s1) w_b(s2) w_c(s3)
 *   B2h[z,t] = sigma [D1 D2 I_ab(s1,s2) J_c(s3) P_3 + D2 D3 I_bc(s2,s3) J_a(s1) P_1 + D1 D3 I_ac(s1,s3) J_b(s2) P_2]
 *   B3h[z,t] = sigma J_a(s1) J_b(s2) J_c(s3) 2 [F2(k1,k2;k3) P_1 P_2 + F2(k2,k3;k1) P_2 P_3 + F2(k3,k1;k2) P_3 P_1]
 * w_x[z,m,s] the weight of a single tracer in hmg_power's cross-spectrum case (matter m u / rho_m0, HOD
 * (u_c Nc + u_s Ns) / ngal, pressure pk) interpolated linearly to the sample, without the scale;
 * I_xy = sum_m wm nzm bh w_x w_y; J_x = (I_x + b_x) - C_x the bracket of P2h in hmg_power (I_x = sum_m wm nzm bh w_x);
 * P_s = Pzk at the sample; k_s = ks[idx] where frac == 0, else (1 - f) ks[idx] + f ks[idx+1] (three rounded operations);
 * D_s = 1 - exp(-(k_s / kstar)^2), or 1 if kstar <= 0; sigma = scale_1 scale_2 scale_3;
 * F2(p,q;r) = 5/7 + mu/2 (p/q + q/p) + 2/7 mu^2, mu = clamp(((r-p)(r+p) - q^2) / (2 p q), -1, 1), evaluated with the longer
 * of (p, q) as p (F2 is symmetric in them; mu then stays within a few ulp for squeezed triangles).  Linear halo bias only.
 * Scales and damping multiply finished sums.  d_Bz (3, nt) = sum_z zweights[z] B[:, z], z in order, needs d_zweights;
 * d_J (3, nz, n) is J by leg.  Any output may be NULL, not all three (d_B NULL with d_Bz: the per-z terms live in a
 * temporary block).  At most one of the three tracers may be an HOD (the 1-halo term of two needs third factorial
 * moments).  The tables and the triangles are checked on the device before any tensor is read through them - the
 * conditions of hmg_trispectrum_1h, a triangle index outside 0 .. n-1, and a triangle that does not close at some z,
 * k_max > (k_mid + k_min)(1 + 2^-40), are errors - and the host waits for that answer: the call synchronises the current
 * stream once and cannot be part of a captured step.  Tracers as for hmg_power (hints and bias overrides are not
 * read).  fp64 on the vector units, every workgroup walks the whole mass axis in order, no atomics: bit-identical on
 * repeat, an element depends only on its own (z, t) entries, not on the other triangles or redshifts of the call.       */
int hmg_bispectrum(hmg_ctx* ctx, int nz, int nm, int nk, int n, int nt,
                   const hmg_tracer* h_a, const hmg_tracer* h_b, const hmg_tracer* h_c,
                   const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm, const double* d_ks,
                   const double* d_Pzk, double rho_m0, double kstar /*<= 0: no damping*/,
                   const int* d_idx /*[nz][n]*/, const double* d_frac, const double* d_scale,
                   const int* d_tri /*[nt][3]*/, const double* d_zweights /*[nz] or NULL*/,
                   double* d_B /*[3][nz][nt] or NULL*/, double* d_Bz /*[3][nt] or NULL*/,
                   double* d_J /*[3][nz][n] or NULL*/);

/* ---- response to a long-wavelength mode and super-sample covariance -------------------------
 * hmg_response: d_R (np, nz, n), the response dP_ab / d delta_b of np spectra (a, b) = h_pairs[2p], h_pairs[2p+1] at the
 * n samples per redshift (tables as for hmg_bispectrum; n <= 256, 1 <= np <= 16):
 *   R[p,z,s] = scale [ (47/21 - n_s/3) P2h + D_s I1 - (beta_a + beta_b) (P2h + D_s A1) ]
 *   A1 = sum_m wm nzm S_ab,  I1 = sum_m wm nzm bh S_ab,  S_ab the sampled square term of hmg_trispectrum_1h without the
 *   scale (first-name-only rules included);  P2h = P_s J_a J_b with J_x, P_s, k_s, D_s of hmg_bispectrum (each leg under
 *   its own name);  n_s the linear interpolant (frac == 0: the node itself) of d_dlnP (nz, nk), the logarithmic slope of
 *   P_lin the caller tabulated;  beta_x = sum_m wm nzm bh (Nc + Ns) / ngal of an HOD leg, 0 of a matter or pressure leg.
 * Scales and damping multiply finished sums.  d_parts (3, np, nz, n) = (A1, I1, P2h), or NULL.  Two HOD tracers in one
 * pair are allowed.  The tables are checked on the device before any tensor is read through them (the conditions of
 * hmg_trispectrum_1h) and the host waits for that answer: the call synchronises the current stream once and cannot be
 * part of a captured step.  Tracers as for hmg_power (hints and bias overrides are not read).  fp64 on the vector units,
 * one thread walks the whole mass axis in order, no atomics: bit-identical on repeat, an element depends only on its own
 * (pair, z, sample), not on the other pairs, samples or redshifts of the call.
 * hmg_ssc: d_cov (np n, np n),  Cov[p n + i, q n + j] = sum_z g[z] r[p,z,i] r[q,z,j],  r[p,z,s] = zscale[p,z] R[p,z,s]
 * (d_zscale NULL: R itself), z in order, each term fma(r r, g, acc): Cov[a,b] has the bits of Cov[b,a].              */
int hmg_response(hmg_ctx* ctx, int nz, int nm, int nk, int n, int np, const hmg_tracer* h_pairs /*[np][2]*/,
                 const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm, const double* d_ks,
                 const double* d_Pzk, const double* d_dlnP /*[nz][nk]*/, double rho_m0, double kstar /*<= 0: no damping*/,
                 const int* d_idx /*[nz][n]*/, const double* d_frac, const double* d_scale,
                 double* d_R /*[np][nz][n]*/, double* d_parts /*[3][np][nz][n] or NULL*/);
int hmg_ssc(hmg_ctx* ctx, int nz, int n, int np, const double* d_R /*[np][nz][n]*/,
            const double* d_zscale /*[np][nz] or NULL*/, const double* d_g /*[nz]*/, double* d_cov /*[np n][np n]*/);

/* ---- the 2-, 3- and 4-halo terms of the trispectrum of two spectra ----------------------------
 * The trispectrum T(k_i, -k_i, k_j, -k_j) of the spectra (a, b) at +-k_i and (c, d) at +-k_j, averaged over the angle
 * between k_i and k_j with a rule of nr <= 256 nodes: d_mu, d_omm = 1 - mu, d_opm = 1 + mu (arrays of their own, formed
 * without cancellation) and weights d_w that sum to 1.  Tables and sampled quantities (w_x, k_s, P_s, J_x, D_s) as for
 * hmg_bispectrum, S_xy as for hmg_trispectrum_1h; n <= 256.
 * hmg_pt_averages: three (nz, n, n) matrices of plain arrays d_ks (nk), d_Pzk (nz, nk), 2 <= nk <= 8192 (the row's ln k and ln P sit in LDS).  Per node,
 *   q-+^2 = (k_i - k_j)^2 + 2 k_i k_j (1 -+ mu)  (never a difference of squares),  P(q) = exp of the linear interpolant of
 *   ln Pzk in ln ks, continued beyond either end with the end panel's slope,  F2 of hmg_bispectrum:
 *   Pbar = sum_t w_t P(q+)
 *   Bbar = sum_t w_t 2 [F2(q+,k_i;k_j) P(q+) P_i + F2(q+,k_j;k_i) P(q+) P_j + F2(k_i,k_j;q+) P_i P_j]
 *   Tbar = sum_t w_t {12 F3s(k_i,-k_i,k_j) P_i^2 P_j + 12 F3s(k_j,-k_j,k_i) P_j^2 P_i
 *                     + sum_{q = q-, q+} 4 P(q) [F2(q,k_j;k_i) P_j + F2(q,k_i;k_j) P_i]^2}
 *   F3s from the recursion for F_n, G_n, symmetrised, orderings with a vanishing partial sum dropped.  Each unordered
 *   pair is evaluated once, its sides ordered by (k, P), and mirrored: the matrices are bit-symmetric.
 * hmg_trispectrum_connected: d_T (5, nz, n, n) = (T1h, T2h13, T2h22, T3h, T4h), with w = wm nzm bh,
 *   I_{x,cd}(i;j) = sum_m w w_x(i) S_cd(j),  I_xy(i,j) = sum_m w s_xy(i,j),  s_xy = w_x(i) w_y(j), or, of twice the same
 *   HOD, [(u_c(i) u_s(j) + u_s(i) u_c(j)) <NcNs> + <Ns(Ns-1)> u_s(i) u_s(j)] / ngal^2 (u at the samples; u_c = 1 without d_cprof):
 *   T1h   = hmg_trispectrum_1h's with d_scale1h (its caller's scale: damping folded in), the same bits
 *   T2h13 = sig D_i D_j {P_i [J_a(i) I_{b,cd} + J_b(i) I_{a,cd}] + P_j [J_c(j) I_{d,ab} + J_d(j) I_{c,ab}]}
 *   T2h22 = sig (D_i D_j)^2 Pbar [I_ac I_bd + I_ad I_bc]
 *   T3h   = sig D_i D_j Bbar [I_ac J_b(i) J_d(j) + I_bd J_a(i) J_c(j) + I_ad J_b(i) J_c(j) + I_bc J_a(i) J_d(j)]
 *   T4h   = sig Tbar J_a(i) J_b(i) J_c(j) J_d(j),       sig = scale_i scale_j
 * Linear halo bias only; three or four galaxies in one halo are formed as w_g S_gg and S_gg S_gg (no third factorial
 * moment).  d_Tz (5, n, n) = sum_z zweights[z] T[:, z], z in order, needs d_zweights; either output may be NULL, not both.
 * All HOD tracers of a call must be the same one.  The tables are checked on the device before any tensor is read
 * through them and the host waits for that answer: neither call can be part of a captured step.  fp64 on the vector
 * units, every workgroup walks the whole mass axis in order, no atomics: bit-identical on repeat, an element depends only
 * on its own (z, i, j) entries.                                                                                        */
int hmg_pt_averages(hmg_ctx* ctx, int nz, int nk, int n, int nr, const double* d_ks, const double* d_Pzk,
                    const int* d_idx /*[nz][n]*/, const double* d_frac,
                    const double* d_mu /*[nr]*/, const double* d_omm, const double* d_opm, const double* d_w,
                    double* d_Pbar /*[nz][n][n]*/, double* d_Bbar, double* d_Tbar);
int hmg_trispectrum_connected(hmg_ctx* ctx, int nz, int nm, int nk, int n, int nr,
                              const hmg_tracer* h_a, const hmg_tracer* h_b, const hmg_tracer* h_c, const hmg_tracer* h_d,
                              const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm,
                              const double* d_ks, const double* d_Pzk, double rho_m0, double kstar /*<= 0: no damping*/,
                              const int* d_idx /*[nz][n]*/, const double* d_frac, const double* d_scale,
                              const double* d_scale1h,
                              const double* d_mu /*[nr]*/, const double* d_omm, const double* d_opm, const double* d_w,
                              const double* d_zweights /*[nz] or NULL*/,
                              double* d_T /*[5][nz][n][n] or NULL*/, double* d_Tz /*[5][n][n] or NULL*/);

/* ---- projected generalised-NFW profiles: gas surface density, optical depth, Compton y --------
 * Row h is one profile f(x) = x^gamma (1 + x^alpha[h])^(-eta[h]), zero beyond x = xcut[h]; gamma > -1 is one number for
 * the call.  d_x holds the projected radii in the rows' scaled units: (n, nr) when per_row_x != 0, else one row of nr shared
 * by every profile.  d_out is (n, nr).  Radii, alpha and xcut must be positive and alpha eta - gamma > 1; the Python layer
 * checks values, these check shapes, kind and gamma.
 * hmg_gnfw_projected, by kind:
 *   HMG_GNFW_SIGMA   F(s) = 2 int_0^sqrt(xcut^2 - s^2) f(sqrt(s^2 + l^2)) dl, exactly 0.0 for s >= xcut;
 *   HMG_GNFW_MEAN    G(s) = (2/s^2) int_0^s F(s') s' ds', the cylinder mass over pi s^2 (N / (pi s^2) for s >= xcut);
 *   HMG_GNFW_EXCESS  G(s) - F(s), the bits of the MEAN result minus the bits of the SIGMA result.
 *   kind | HMG_GNFW_GENERAL evaluates rows with alpha == 1 like any other row (testing; they have a shorter evaluation).
 *   Gauss-Legendre with 64 nodes in t, l = s sinh t, and in v, r = s v^2; one thread per output.
 * hmg_gnfw_projected_smooth: kind HMG_GNFW_SIGMA only; F convolved with a circular Gaussian of width d_sigma[h] > 0 in the
 *   same units, int ds' (s'/sig^2) exp(-(s - s')^2 / 2 sig^2) I0e(s s'/sig^2) F(s'); one wavefront per output.
 * Both run on the current stream, fp64, fixed summation order, no atomics: bit-identical on repeat, and an output depends
 * only on its own row and radius.  The first call on a device uploads the node table and so cannot be inside a captured
 * step.
 * hmg_gnfw_quad_table: the node table on the host (no device needed), HMG_GNFW_TABLE_DOUBLES doubles: u[64], w[64]
 *   (Gauss-Legendre on [0, 1]), u^2, 2 ln u, 2 u w (the inner sphere), then for the 32-node rule U, W of the smoothing
 *   sin^2(pi U / 2), cos^2(pi U / 2), W (pi/2) sin(pi U).                                                            */
#define HMG_GNFW_SIGMA 0
#define HMG_GNFW_MEAN 1
#define HMG_GNFW_EXCESS 2
#define HMG_GNFW_GENERAL 4
#define HMG_GNFW_TABLE_DOUBLES 416
int hmg_gnfw_projected(hmg_ctx* ctx, int n, int nr, int per_row_x, int kind, const double* d_alpha, const double* d_eta,
                       const double* d_xcut, double gamma, const double* d_x, double* d_out);
int hmg_gnfw_projected_smooth(hmg_ctx* ctx, int n, int nr, int per_row_x, int kind, const double* d_alpha,
                              const double* d_eta, const double* d_xcut, double gamma, const double* d_x,
                              const double* d_sigma, double* d_out);
int hmg_gnfw_quad_table(double* h_table /*[HMG_GNFW_TABLE_DOUBLES]*/);

/* ---- redshift-space spectra of the dispersion halo model --------------------------------------
 * One pair of tracers (a, b), matter or HOD (a pressure tracer is an error), at n nodes d_kindex (n) of the k grid,
 * 1 <= n <= nk, the same for every redshift, and nmu values of mu, 1 <= nmu <= 32.  A species of a leg at (z, m, k) is a
 * pair (value, alpha): (m/rho_m0 u, alpha_m) of a matter name; (Nc/ngal (u_c or 1), alpha_c) and (Ns/ngal u_s, alpha_s)
 * of an HOD.  With x = k sigma_s[z,m] (d_sigma (nz, nm) >= 0, comoving Mpc) the weight of a leg is
 *   w^s(mu) = sum_species value exp(-alpha^2 x^2 mu^2 / 2).
 * hmg_rsd_wedges: d_out (2, nz, n, nmu) = (P1h, P2h),
 *   P1h = damp[s] sum_m wm nzm S^s,  S^s = w^s_a w^s_b, or of two HOD tracers the first one's
 *         2<NcNs>/ngal^2 u_c u_s exp(-(alpha_c^2 + alpha_s^2) x^2 mu^2 / 2) + <Ns(Ns-1)>/ngal^2 u_s^2 exp(-alpha_s^2 x^2 mu^2);
 *   P2h = P_lin (J^s_a + f mu^2 K^s_a) (J^s_b + f mu^2 K^s_b),  J^s = (I^s + b) - C,  K^s = (V^s + 1) - C0,
 *         I^s = sum_m wm nzm bh w^s,  V^s = sum_m wm nzm w^s,  C, C0 the same two sums of the k -> 0 weight without a
 *         Gaussian, b = 1 of a matter tracer and the HOD bias sum of an HOD - operation by operation in this order.
 *   d_damp (n) is the factor of the 1-halo term (the caller's damping, or ones), d_f (nz) the growth rate.
 *   d_parts (4, nz, n, nmu) = (I^s_a, V^s_a, I^s_b, V^s_b), or NULL.
 * hmg_rsd_multipoles: d_out (2, nz, n, 3), the multipoles l = 0, 2, 4 of the two terms.  The 1-halo ones are exact in mu:
 *   Q_n = sum_m wm nzm sum_terms value M_n(t),  M_n(t) = int_0^1 mu^2n exp(-t mu^2) dmu (csrc/gauss_moments.hpp), t the
 *   exponent's factor of mu^2;  P_0 = Q_0, P_2 = 5/2 (3 Q_1 - Q_0), P_4 = 9/8 ((35 Q_2 - 30 Q_1) + 3 Q_0), times d_damp.
 *   d_Q (3, nz, n) = Q_n, or NULL.  The 2-halo ones are the rule sum_q d_wl[l][q] P2h(mu_q), q ascending, over the nmu nodes
 *   d_mus with the weights d_wl (3, nmu) = (2l + 1) w_q L_l(mu_q) the caller tabulated.
 * The table is checked on the device before any tensor is read through it and the host waits for that answer: a call
 * synchronises the current stream once and cannot be part of a captured step.  Tracers as for hmg_power (hints and bias
 * overrides are not read).  fp64 on the vector units, one thread walks the whole mass axis in order, no atomics:
 * bit-identical on repeat, an element depends only on its own (z, sample, mu), not on the rest of the call.            */
int hmg_rsd_wedges(hmg_ctx* ctx, int nz, int nm, int nk, int n, int nmu, const hmg_tracer* h_a, const hmg_tracer* h_b,
                   const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm, const double* d_ks,
                   const double* d_Pzk, double rho_m0, const int* d_kindex /*[n]*/, const double* d_damp /*[n]*/,
                   const double* d_mus /*[nmu]*/, const double* d_sigma /*[nz][nm]*/, const double* d_f /*[nz]*/,
                   double alpha_m, double alpha_c, double alpha_s, double* d_out /*[2][nz][n][nmu]*/,
                   double* d_parts /*[4][nz][n][nmu] or NULL*/);
int hmg_rsd_multipoles(hmg_ctx* ctx, int nz, int nm, int nk, int n, int nmu, const hmg_tracer* h_a, const hmg_tracer* h_b,
                       const double* d_nzm, const double* d_bh, const double* d_ms, const double* d_wm, const double* d_ks,
                       const double* d_Pzk, double rho_m0, const int* d_kindex /*[n]*/, const double* d_damp /*[n]*/,
                       const double* d_mus /*[nmu]*/, const double* d_wl /*[3][nmu]*/, const double* d_sigma /*[nz][nm]*/,
                       const double* d_f /*[nz]*/, double alpha_m, double alpha_c, double alpha_s,
                       double* d_out /*[2][nz][n][3]*/, double* d_Q /*[3][nz][n] or NULL*/);

/* ---- one-point statistics of a field that is a sum of halo profiles on the sky ----------------
 * A sample is ring t of a halo (z, m): its signal s = d_signal[z][m][t], or d_amp[z][m] d_signal[z][m][t] (one rounded
 * product) where d_amp is not NULL, and its weight W = ((d_zw[z] d_wm[m]) d_nzm[z][m]) d_area[z][m][t], rounded in this
 * order.  Both entry points sum over the samples of the mass window m_lo <= m < m_hi (0 <= m_lo < m_hi <= nm) and every t.
 * hmg_onepoint_exponent: the exponent of the characteristic function of Poisson-placed halos on the uniform grid
 *   lambda_j = j dlambda, j < nlambda (dlambda finite and positive):
 *     A[z][j] = sum W (exp(i lambda_j s) - 1),  Re = sum W (-2 sin^2(lambda_j s / 2)),  Im = sum W sin(lambda_j s),
 *   the row z already multiplied by d_zw[z].  d_rows (nz, 2, nlambda): plane 0 of a row is the real part, plane 1 the
 *   imaginary part.  d_total (2, nlambda) = sum_z d_rows[z], z ascending, or NULL.  A[z][0] is exactly 0 (written, not summed).
 * hmg_onepoint_moments: d_rows (nz, 4), d_rows[z][p - 1] = sum W s^p, p = 1 .. 4 - the cumulants of the same field;
 *   d_total (4) their sum over z, or NULL.
 * fp64 on the vector units, sines and cosines by sici.hpp's reduction below 2^30 rad and the library's beyond, no atomics.
 * The order of every addition depends on (m_hi - m_lo, nt) alone: bit-identical on repeat, and a row has the bits of the
 * call with that redshift alone.  Launch-only on the current stream (the exponent takes one temporary block from the
 * context's allocator when the window holds more than 4096 samples).                                                   */
int hmg_onepoint_exponent(hmg_ctx* ctx, int nz, int nm, int nt, const double* d_signal /*[nz][nm][nt]*/,
                          const double* d_area /*[nz][nm][nt]*/, const double* d_amp /*[nz][nm] or NULL*/,
                          const double* d_nzm /*[nz][nm]*/, const double* d_wm /*[nm]*/, const double* d_zw /*[nz]*/,
                          int m_lo, int m_hi, int nlambda, double dlambda, double* d_rows /*[nz][2][nlambda]*/,
                          double* d_total /*[2][nlambda] or NULL*/);
int hmg_onepoint_moments(hmg_ctx* ctx, int nz, int nm, int nt, const double* d_signal, const double* d_area,
                         const double* d_amp, const double* d_nzm, const double* d_wm, const double* d_zw, int m_lo,
                         int m_hi, double* d_rows /*[nz][4]*/, double* d_total /*[4] or NULL*/);

/* ---- HOD parameter ensembles: P_gg and P_gm of S parameter sets at once -----------------------
 * Set s is d_par[s] = (sig_log_mstellar, alphasat, Bsat, betasat, Bcut, betacut); corr (0 = max, 1 = min) holds for the
 * whole call; d_lthr (S, nz) are the thresholds log10 M*_thr.  Centrals sit at the halo centre (u_c = 1).
 * hmg_hod_ensemble: the occupations and sums of hmg_hod for every set.  log10 M*(z, m), the SHMR inversion, is evaluated
 *   once per (z, m) and shared by the sets; a point runs hmg_hod's operations in hmg_hod's order and the sums keep its tile
 *   order per set, so every number has the bits hmg_hod gives for that set alone.  d_ngal, d_bg (S, nz).  d_occ
 *   (4, S, nz, nm) = (Nc, Ns, NsNsm1, NcNs), or NULL.  d_coef, or NULL, is the block the second call reads, of
 *   4 nz nm Spad + S nz doubles with Spad = S rounded up to a multiple of 8:
 *     coef[nz][nm][Spad][4] = (Nc, Ns, 2 NcNs, NsNsm1), zeros in the sets S .. Spad-1;  then
 *     craw[S][nz] = sum_m ((wm nzm) bh) (Nc + Ns), in the tile order of the n_gal sum.
 *   With both NULL nothing of size S nz nm is written (the mode of a bisection on n_gal).  Launch-only.
 * hmg_hod_ensemble_power: d_out (4, S, nz, n) = (P1h_gg, P2h_gg, P1h_gm, P2h_gm) at n columns, the nodes d_kindex (n) of the
 *   k grid (any order, repeats allowed) or, with d_kindex NULL, the whole grid (n = nk).  d_us is the satellite tensor,
 *   d_um the matter tensor of the cross spectrum (the same pointer: the tensor is loaded once).  With w = wm nzm:
 *     G = sum_m (2 NcNs) (w u_s) + NsNsm1 ((w u_s) u_s),   X = sum_m (Ns u_s + Nc) ((w m/rho_m0) u_m),
 *     I = sum_m (Ns u_s + Nc) (w bh),   I_m = sum_m ((w bh) m/rho_m0) u_m,   one FMA chain each, m ascending;  then
 *     G / ngal^2, X / ngal, I / ngal, C = craw / ngal, J_g = (I + bg) - C, J_m = (I_m + 1) - C_m,
 *     P1h_gg = damp G, P2h_gg = (Pzk J_g) J_g, P1h_gm = damp X, P2h_gm = (Pzk J_g) J_m
 *   - every 1/ngal on the finished sums.  d_damp (n) is the factor of the 1-halo terms (the caller's damping, or ones).
 *   d_parts (3, S, nz, n) = (G, X, I) after their divisions, or NULL.  A given d_kindex is checked on the device before any
 *   tensor is read through it and the host waits for that answer: the call then synchronises the current stream once and
 *   cannot be part of a captured step.  fp64 on the vector units, no atomics: bit-identical on repeat, an element depends
 *   only on its own (set, z, node), not on which other sets, nodes or redshifts the call holds.                          */
int hmg_hod_ensemble(hmg_ctx* ctx, int S, int nz, int nm, int corr, const double* d_par /*[S][6]*/,
                     const double* d_lthr /*[S][nz]*/, const double* d_zs, const double* d_ms, const double* d_nzm,
                     const double* d_bh, const double* d_wm, double* d_ngal /*[S][nz]*/, double* d_bg /*[S][nz]*/,
                     double* d_occ /*[4][S][nz][nm] or NULL*/, double* d_coef /*the coefficient block or NULL*/);
int hmg_hod_ensemble_power(hmg_ctx* ctx, int S, int nz, int nm, int nk, int n, const double* d_us, const double* d_um,
                           const double* d_coef, const double* d_ngal, const double* d_bg, const double* d_nzm,
                           const double* d_bh, const double* d_ms, const double* d_wm, const double* d_ks,
                           const double* d_Pzk, double rho_m0, const int* d_kindex /*[n] or NULL*/,
                           const double* d_damp /*[n]*/, double* d_out /*[4][S][nz][n]*/,
                           double* d_parts /*[3][S][nz][n] or NULL*/);

/* ---- cluster number counts: the survey selection in bins of significance, summed over the mass function (section 25) --
 * A halo (z, m) has the mean log-observable mu = d_lnobs[z][m] and the log-normal scatter sg = d_sigln[z][m]; tile tau of
 * the survey has the solid angle d_area[tau] and the noise exp(d_lnnoise[tau]); the nq bins are [d_edges[a], d_edges[a+1]).
 * kind 0 (gaussian): with the rule (d_t, d_w) of G nodes for the unit normal,
 *     S_a[z][m] = sum_tau sum_g (area[tau] w[g]) P_a(q),  q = exp((mu + sg t[g]) - lnnoise[tau]),
 *     P_a(q) = 1/2 [erfc(ua) - erfc(ub)],  ua = (e_a - q) / sqrt 2,  ub = (e_a+1 - q) / sqrt 2,
 *   formed as 1/2 [erfc(-ub) - erfc(-ua)] where (e_a - q) + (e_a+1 - q) < 0; erfc of a negative argument is 2 - erfc of its
 *   magnitude, so every edge costs one erfc.  The edges may be -inf and +inf.
 * kind 1 (none): S_a[z][m] = sum_tau area[tau] P_a with ua = (ln e_a - xi) / (sqrt 2 sg), xi = mu - lnnoise[tau], the
 *   same two forms; d_t, d_w and G are not read (G >= 1), sg must be positive and the edges not negative.
 * d_n[z][a] = sum_m d_wm[m] (d_nzm[z][m] S_a), d_bn[z][a] = sum_m (d_wm[m] (d_nzm[z][m] S_a)) d_bh[z][m] over the window
 * m_lo <= m < m_hi (0 <= m_lo < m_hi <= nm).  d_S (nz, nm, nq), or NULL: S_a itself, zero outside the window; with NULL
 * nothing of that size exists.  No term is skipped.  fp64 on the vector units, no atomics, the order of every sum fixed
 * (kernels/clusters.hpp): bit-identical on repeat, and an element depends on its own (z, bin) only - not on the other bins
 * or redshifts of the call.  Launch-only (one temporary block of 2 nz ceil(nm / 64) nq doubles from the context).        */
int hmg_cluster_selection(hmg_ctx* ctx, int nz, int nm, int T, int G, int nq, int kind, const double* d_lnobs /*[nz][nm]*/,
                          const double* d_sigln /*[nz][nm]*/, const double* d_lnnoise /*[T]*/, const double* d_area /*[T]*/,
                          const double* d_t /*[G]*/, const double* d_w /*[G]*/, const double* d_edges /*[nq+1]*/, int m_lo,
                          int m_hi, const double* d_nzm, const double* d_bh, const double* d_wm, double* d_n /*[nz][nq]*/,
                          double* d_bn /*[nz][nq]*/, double* d_S /*[nz][nm][nq] or NULL*/);

/* ---- the CIB halo model: luminosities and the spectra of every pair of frequencies -------------
 * hmg_cib_luminosity: d_Lc, d_Ls (F, nz, nm), the emissivity weights of the centrals and the satellites of a Shang et al.
 *   (2012) model at the observed frequencies d_nus [GHz], F <= HMG_CIB_FMAX.  h_par = (alpha, T0 [K], beta, gamma, delta,
 *   z_p, log10 M_eff, sigma2, M_min, L0, x0); x0 is the root of x / (1 - exp(-x)) = 3 + beta + gamma.  With
 *     L(M, z; nu) = L0 Phi(z) Sigma(M) Theta((1+z) nu, T0 (1+z)^alpha),   Phi = min(1+z, 1+z_p)^delta,
 *     Sigma(M) = M (2 pi sigma2)^-1/2 exp(-(log10 M - log10 M_eff)^2 / (2 sigma2)),   nu0 = x0 k T / h,
 *     Theta = (nu/nu0)^(3+beta) expm1(x0) / expm1(h nu / k T) below nu0, (nu/nu0)^-gamma from nu0 on,
 *   L_c = L(ms[m]) / 4 pi where ms[m] >= M_min, else 0;  L_s = sum_g (w[g] hw) N(q_g) L(m_g) / 4 pi, g ascending, over
 *   the rule (d_t, d_w) of nsub nodes on [0, 1] mapped to ln m in [ln M_min, ln ms[m]]: hw = ln(ms[m] / M_min),
 *   m_g = M_min exp(hw t[g]), q = m_g / ms[m], N = 0.3 q^-0.7 exp(-9.9 q^2.5); 0 where ms[m] <= M_min.  d_scut (F), or
 *   NULL: a source - a central, or a subhalo node - with L / (4 pi (1+z) chi^2) > d_scut[f] is masked (its L is 0);
 *   d_chis (nz) [Mpc].  The order of every operation is written down in kernels/cib.hpp.  Launch-only, no temporaries.
 * hmg_emission_power: the mass integrals of the emissivity tracers a_f = L_c[f] + L_s[f] u_s at n columns, the nodes
 *   d_kindex (n) of the k grid or, with d_kindex NULL, the whole grid (n = nk), as hmg_hod_ensemble_power takes them.
 *   With w = wm nzm, t_f = L_s[f] u_s:
 *     d_P1h[pair][z][col] = damp sum_m w (L_c[f] t_g + L_c[g] t_f + t_f t_g),  pair = f F - f (f - 1) / 2 + (g - f), f <= g;
 *     d_I[f][z][col]      = sum_m (w bh) a_f        (the 2-halo leg: P2h_fg = Pzk I_f I_g, no consistency term);
 *     d_X1h[p][f][z][col] = damp sum_m w a_f c_p prof_p   for the NP <= 2 partners h_partners[p]: matter (c = m / rho_m0)
 *       or pressure (c = 1) tracers; any other kind is refused.  A partner's hints are not read: a tensor with a pending
 *       left fill is filled by the caller first (hmg_prefix_fill).  NP = 0: h_partners and d_X1h may be NULL.
 *   The pair term is never formed as a_f a_g - L_c[f] L_c[g].  fp64 on the vector units, no atomics, one FMA chain over
 *   m per element: bit-identical on repeat, and an element does not depend on which other frequencies, pairs, partners,
 *   nodes or redshifts the call holds (in a pair, f is the frequency that comes first).  d_us and a partner tensor equal
 *   to it are loaded once.  A given d_kindex is checked on the device first and the host waits for that answer (not in a
 *   captured step).  Temporaries: one block of 8 nz nm (2 Fpad + 4) + 64 bytes from the context, Fpad = F rounded up to 4. */
#define HMG_CIB_FMAX 16
#define HMG_CIB_NPAR 11
int hmg_cib_luminosity(hmg_ctx* ctx, int F, int nz, int nm, int nsub, const double* d_nus /*[F]*/, const double* d_zs,
                       const double* d_ms, const double* d_chis /*[nz]*/, const double* d_scut /*[F] or NULL*/,
                       const double* d_t /*[nsub]*/, const double* d_w /*[nsub]*/, const double h_par[HMG_CIB_NPAR],
                       double* d_Lc /*[F][nz][nm]*/, double* d_Ls /*[F][nz][nm]*/);
int hmg_emission_power(hmg_ctx* ctx, int F, int nz, int nm, int nk, int n, const double* d_us, const double* d_Lc,
                       const double* d_Ls, int NP, const hmg_tracer* h_partners /*[NP] or NULL*/, const double* d_nzm,
                       const double* d_bh, const double* d_ms, const double* d_wm, double rho_m0,
                       const int* d_kindex /*[n] or NULL*/, const double* d_damp /*[n]*/, double* d_P1h /*[npair][nz][n]*/,
                       double* d_I /*[F][nz][n]*/, double* d_X1h /*[NP][F][nz][n] or NULL*/);

/* ---- z-slab gather over RCCL/xGMI-------------------------------------------------
 * One communicator per context.  The 128-byte id comes from hmg_comm_unique_id on rank 0
 * and is distributed by the caller (file, socket, MPI, ...).                                     */
#define HMG_COMM_ID_BYTES 128
int hmg_comm_unique_id(char h_id[HMG_COMM_ID_BYTES]);
int hmg_comm_init(hmg_ctx* ctx, const char h_id[HMG_COMM_ID_BYTES], int rank, int nranks);
int hmg_comm_allgather(hmg_ctx* ctx, const double* d_send, double* d_recv, size_t count_per_rank);
/* n gathers of count_per_rank doubles each, fused into one RCCL group launch. */
int hmg_comm_allgather_multi(hmg_ctx* ctx, int n, const double* const* h_d_send,
                             double* const* h_d_recv, size_t count_per_rank);
/* The gather of one pass off the compute stream: record ready_slot on the current lane, make
 * comm_lane wait for it, issue the grouped all-gather there and record done_slot.  A later
 * hmg_event_wait(done_slot) on the compute lane orders the next overwrite of the send buffers.   */
int hmg_comm_gather_async(hmg_ctx* ctx, int n, const double* const* h_d_send, double* const* h_d_recv,
                          size_t count_per_rank, int ready_slot, int done_slot, int comm_lane);
/* Slabs of unequal length (nz not a multiple of the number of ranks: SURVEY 8e partitions "contiguous z-slabs";
 * the README grid has nz = 20, /root/reference/README.rst:55): rank r contributes h_counts[r] doubles per array,
 * which land at the prefix-sum offset of every rank's receive buffer - one ncclBroadcast per (array, rank) in one
 * group launch.  h_counts has one entry per rank and must be the same on every rank; equal counts take the
 * all-gather of the entry points above. */
int hmg_comm_allgatherv_multi(hmg_ctx* ctx, int n, const double* const* h_d_send, double* const* h_d_recv,
                              const size_t* h_counts);
int hmg_comm_gatherv_async(hmg_ctx* ctx, int n, const double* const* h_d_send, double* const* h_d_recv,
                           const size_t* h_counts, int ready_slot, int done_slot, int comm_lane);
/* rank and size as RCCL reports them (ncclCommUserRank / ncclCommCount); 0 and 1 without a communicator */
int hmg_comm_info(hmg_ctx* ctx, int* h_rank, int* h_nranks);
int hmg_comm_barrier(hmg_ctx* ctx);     /* blocks */
int hmg_comm_destroy(hmg_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* HMGRID_H */
