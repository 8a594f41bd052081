/* geosrad.h -- C ABI of the MI355X-native radiation hot path (libgeosrad.so).
 *
 * Drop-in boundary: these entry points are what a Fortran ISO_C_BINDING shim binds in place of the
 * reference's solver entry points (paths relative to the GEOS-ESM/GEOSradiation_GridComp checkout):
 *
 *   geosrad_rrtmg_lw[_dev]        <- rrtmg_lw_rad::rrtmg_lw
 *                                    GEOSirrad_GridComp/RRTMG/rrtmg_lw/gcm_model/src/rrtmg_lw_rad.F90:15-23,110-201
 *   geosrad_set_tables_lw         <- rrtmg_lw_init::rrtmg_lw_ini           .../src/rrtmg_lw_init.F90:22
 *   geosrad_rrtmg_sw[_dev]        <- rrtmg_sw_rad::rrtmg_sw
 *   geosrad_rrtmg_sw_radval[_dev] <- rrtmg_sw_rad::rrtmg_sw built with -DSOLAR_RADVAL
 *                                    GEOSsolar_GridComp/RRTMG/rrtmg_sw/gcm_model/src/rrtmg_sw_rad.F90:68-124
 *   geosrad_set_tables_sw         <- rrtmg_sw_init::rrtmg_sw_ini           .../src/rrtmg_sw_init.F90:23
 *   geosrad_irrad[_dev]           <- irradmod::irrad                       GEOSirrad_GridComp/irrad.F90:27-35
 *   geosrad_sorad[_dev]           <- soradmod::sorad                       GEOSsolar_GridComp/sorad.F90:43-51
 *   geosrad_sorad_na[_dev]        <- the same + its aerosol-free fluxes    GEOS_SolarGridComp.F90:3249-3259, :3997-4016
 *   geosrad_set_tables_chou_sw    <- sorad_constants / rad_constants (data modules)  GEOSsolar_GridComp/soradconstants.F90
 *   geosrad_set_tables_chou_lw    <- irrad_constants / rad_constants (data modules)  GEOSirrad_GridComp/irradconstants.F90
 *   geosrad_mcica[_dev]           <- cloud_subcol_gen::generate_stochastic_clouds
 *                                    GEOS_RadiationShared/cloud_subcol_gen.F90:132-137
 *   geosrad_clearcounts           <- cloud_subcol_gen::clearCounts_threeBand   .../cloud_subcol_gen.F90:611-614
 *   geosrad_set_corr_lengths      <- cloud_subcol_gen::initialize_cloud_subcol_gen .../cloud_subcol_gen.F90:109-111
 *   geosrad_set_inhomogeneity     <- cloud_condensate_inhomogeneity::{set,unset}_inhomogeneity
 *                                    GEOS_RadiationShared/cloud_condensate_inhomogeneity.F90:45,75
 *
 * Conventions
 *   - One context per (process, GPU, precision).  `real_kind` = 4 or 8 fixes the element type of every
 *     `const void*`/`void*` real array below (float or double), like the reference's default `real`.
 *   - Array layouts are exactly the reference's Fortran layouts, e.g. play(ncol,nlay): column index
 *     fastest; RRTMG ordering (layer 1 = lowest layer).  Nothing is transposed at the boundary.
 *   - Plain entry points take caller-owned HOST pointers (copied to/from HBM internally); `_dev` entry
 *     points take DEVICE pointers and a hipStream_t (as void*) and are asynchronous on that stream.
 *   - Every function returns 0 on success or a GEOSRAD_E* code; geosrad_last_error() gives the text.
 *     Where the reference would `error stop`, the code is GEOSRAD_EINPUT and the text is the reference's
 *     message (e.g. "negative values in input: play", rrtmg_lw_rad.F90:209-318).
 *   - Thread safety: a context may be used by one thread at a time; distinct contexts are independent
 *     (the reference's module-level state is replaced by the context).
 */
#ifndef GEOSRAD_H
#define GEOSRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct geosrad_ctx geosrad_ctx;

enum {
    GEOSRAD_OK = 0,
    GEOSRAD_EINVAL = 1,   /* bad argument / call order                                   */
    GEOSRAD_ENODEV = 2,   /* no usable HIP device: the product never falls back to CPU */
    GEOSRAD_EHIP = 3,     /* HIP runtime error                                          */
    GEOSRAD_ETABLE = 4,   /* malformed / missing coefficient table                      */
    GEOSRAD_EINPUT = 5,   /* the reference would `error stop` on these inputs           */
    GEOSRAD_ENOMEM = 6
};

/* NB_LW = nbndlw, NG_LW = ngptlw (parrrtm.F90:33,39) */
#define GEOSRAD_NB_LW 16
#define GEOSRAD_NG_LW 140

/* ---- context ------------------------------------------------------------------------------------
 * The reference keeps its state in module variables of the process; here it lives in a context.  One context = one HIP
 * device (geosrad_create) or several (geosrad_create_multi, SURVEY 8b: the host-pointer solver entry points then cut [0, ncol) into
 * contiguous shards, one per device, processed concurrently; results bitwise those of one device).
 * device_id = GEOSRAD_DEVICE_AUTO: the device geosrad_pick_device chooses - GEOSRAD_DEVICE if set (taken as it is: an id outside
 * [0, ndev) is GEOSRAD_ENODEV, not another GPU), else the launcher's node-local MPI rank (OMPI_COMM_WORLD_LOCAL_RANK, SLURM_LOCALID,
 * MV2_COMM_WORLD_LOCAL_RANK, MPI_LOCALRANKID, PMI_LOCAL_RANK) modulo the number of visible devices - what the Fortran drop-in uses, so the ranks of a GEOS job (GEOS_SolarGridComp.F90:3701-3709 balances their
 * work) spread over a node's GPUs without configuration. */
#define GEOSRAD_DEVICE_AUTO (-1)
int geosrad_create(geosrad_ctx **ctx, int device_id, int real_kind /* 4 | 8 */);
int geosrad_create_multi(geosrad_ctx **ctx, const int *device_ids, int ndev, int real_kind);
int geosrad_pick_device(int ndev);      /* pure function of the environment; no device needed; -1 = GEOSRAD_DEVICE out of range */
int geosrad_destroy(geosrad_ctx *ctx);
const char *geosrad_last_error(const geosrad_ctx *ctx);
int geosrad_real_kind(const geosrad_ctx *ctx);
/* max columns processed per internal batch (bounds the HBM workspace); default 131072 */
int geosrad_set_chunk(geosrad_ctx *ctx, int max_columns);
/* bytes of HBM workspace currently held (the second set of RRTMG_LW band partials of the RATS / aerosol-free passes included) */
size_t geosrad_workspace_bytes(const geosrad_ctx *ctx);
/* Chou-Suarez cloud mode: the reference's -DOVERCAST build of irrad.F90 / sorad.F90 (a layer is clear or fully cloudy; random overlap of
 * the cloudy layers; sorad's cloud optical thickness not scaled; ict / icb not read).  One flag per scheme (GEOS compiles them in separate
 * components); 0 (the default) = maximum-random overlap.  Applies to geosrad_irrad[_dev], geosrad_sorad[_dev],
 * geosrad_lw_driver_chou_dev and geosrad_sw_driver_chou_dev, on every device of a multi-device context.  Unknown bits: GEOSRAD_EINVAL, the mode unchanged. */
enum { GEOSRAD_OVERCAST_IRRAD = 1, GEOSRAD_OVERCAST_SORAD = 2 };
int geosrad_set_overcast(geosrad_ctx *ctx, int flags);
int geosrad_get_overcast(const geosrad_ctx *ctx);

/* ---- tables ("GRTB" blobs, geosradiation_gridcomp_amd/data/) ------------------------------------- */
/* what rrtmg_lw_ini leaves in rrlw_kgNN/rrlw_tbl/rrlw_wvn/rrlw_ref/rrlw_cld (rrtmg_lw_init.F90:22-165) */
int geosrad_set_tables_lw(geosrad_ctx *ctx, const void *blob, size_t nbytes);
int geosrad_load_tables_lw(geosrad_ctx *ctx, const char *path);
/* what rrtmg_sw_ini leaves in rrsw_kgNN/rrsw_ref/rrsw_cld/rrsw_wvn/NRLSSI2 (SW/rrtmg_sw_init.F90:23-190) */
int geosrad_set_tables_sw(geosrad_ctx *ctx, const void *blob, size_t nbytes);
int geosrad_load_tables_sw(geosrad_ctx *ctx, const char *path);
/* the coefficient tables of the Chou-Suarez LW scheme: irrad_constants + the IR part of rad_constants */
int geosrad_set_tables_chou_lw(geosrad_ctx *ctx, const void *blob, size_t nbytes);
int geosrad_load_tables_chou_lw(geosrad_ctx *ctx, const char *path);
/* the coefficient tables of the Chou-Suarez SW scheme: sorad_constants + the UV / NIR part of rad_constants */
int geosrad_set_tables_chou_sw(geosrad_ctx *ctx, const void *blob, size_t nbytes);
int geosrad_load_tables_chou_sw(geosrad_ctx *ctx, const char *path);
/* ih = 0 homogeneous (blob ignored), 1 beta, 2 gamma; blob = xcw(1000,140) table of that kind */
int geosrad_set_inhomogeneity(geosrad_ctx *ctx, int ih, const void *xcw_blob, size_t nbytes);
int geosrad_load_inhomogeneity(geosrad_ctx *ctx, int ih, const char *path);
/* adl = (am1, am2, am30, am4) cloud presence, rdl = same for condensate; NULL keeps the current value */
int geosrad_set_corr_lengths(geosrad_ctx *ctx, const double *adl, const double *rdl);
/* host copy of one named real array of a *.grtb coefficient file; needs neither a context nor a device.  The Fortran shim uses
 * it for the xcw table behind the reference's host function zcw_lookup (cloud_condensate_inhomogeneity.F90:86-124), which
 * GEOS_IrradGridComp.F90:1472 / GEOS_SolarGridComp.F90:3346 import.  count = number of reals expected (checked). */
int geosrad_read_table(const char *path, const char *name, int real_kind, void *dst, size_t count);

/* ---- RRTMG_LW --------------------------------------------------------------------------------------
 * Argument names, order, units and meaning are those of rrtmg_lw (rrtmg_lw_rad.F90:15-201).
 *   in : play,tlay,h2ovmr..ccl4vmr,cldf,ciwp,clwp,rei,rel,zm (ncol,nlay); plev,tlev (ncol,0:nlay);
 *        tsfc,alat (ncol); emis (ncol,16); tauaer (ncol,nlay,16); band_output[16] (0/1)
 *   out: uflx,dflx,uflxc,dflxc,duflx_dTs,duflxc_dTs (ncol,nlay+1); clearCounts int32 (ncol,4);
 *        olrb,dolrb_dTs (16,ncol) [touched only for bands with band_output != 0]
 * psize (cache-blocking partition size) is accepted for signature compatibility and ignored.
 * duflx*_dTs / dolrb_dTs may be NULL when dudTs == 0.  tauaer == NULL means "no aerosol" (all zero). */
int geosrad_rrtmg_lw(geosrad_ctx *ctx, int ncol, int nlay, int psize, int dudTs,
                     const void *play, const void *plev, const void *tlay, const void *tlev,
                     const void *tsfc, const void *emis,
                     const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr,
                     const void *n2ovmr, const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr,
                     const void *cfc22vmr, const void *ccl4vmr,
                     const void *cldf, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                     int iceflglw, int liqflglw,
                     const void *tauaer, const void *zm, const void *alat, int dyofyr, int cloudLM, int cloudMH,
                     int32_t *clearCounts,
                     void *uflx, void *dflx, void *uflxc, void *dflxc, void *duflx_dTs, void *duflxc_dTs,
                     const int32_t *band_output, void *olrb, void *dolrb_dTs);

/* same, all array pointers in device memory; asynchronous on `stream` (hipStream_t).  Input validation
 * results (the reference's error stops) are reported by geosrad_check(). */
int geosrad_rrtmg_lw_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlay, int psize, int dudTs,
                         const void *play, const void *plev, const void *tlay, const void *tlev,
                         const void *tsfc, const void *emis,
                         const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr,
                         const void *n2ovmr, const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr,
                         const void *cfc22vmr, const void *ccl4vmr,
                         const void *cldf, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                         int iceflglw, int liqflglw,
                         const void *tauaer, const void *zm, const void *alat, int dyofyr, int cloudLM, int cloudMH,
                         int32_t *clearCounts,
                         void *uflx, void *dflx, void *uflxc, void *dflxc, void *duflx_dTs, void *duflxc_dTs,
                         const int32_t *band_output /* host */, void *olrb, void *dolrb_dTs);

/* Synchronise `stream` and translate the device-side input checks of the preceding *_dev calls into a
 * return code (GEOSRAD_OK / GEOSRAD_EINPUT + message).  The host-pointer entry points call this. */
int geosrad_check(geosrad_ctx *ctx, void *stream);

/* Per-kernel timing with HIP events recorded on the launch stream, around every kernel the *_dev entry points
 * enqueue (kernel ids 0..5 = k_validate_pwv, k_setcoef, k_overlap, k_mcica, k_lw_bands, k_lw_reduce; 6..9 =
 * k_sw_validate, k_sw_setcoef, k_sw_bands, k_sw_reduce; 10..11 = k_chou_prep, k_chou_bands; 12..13 = k_sorad_prep (+ cloud), k_sorad_pass; k_overlap / k_mcica are shared).
 * geosrad_profile(ctx, 1) resets and enables, geosrad_profile_read() waits for the recorded events and
 * returns the accumulated milliseconds and launch count of one kernel. */
int geosrad_profile(geosrad_ctx *ctx, int enable);
int geosrad_profile_read(geosrad_ctx *ctx, int kernel_id, double *total_ms, long *launches);
const char *geosrad_kernel_name(int kernel_id);      /* the slot's generic name (the default path's first mapping) */
/* the kernel that runs in that slot under the context's kernel paths, as it is named in a rocprofv3 kernel trace
 * (k_sw_reform | k_sw_bands, k_lw_bands | k_lw_cols, k_sorad_pass | k_sorad_col ...) */
const char *geosrad_kernel_label(geosrad_ctx *ctx, int kernel_id);

/* Test hook (host pointers, n doubles each): a / b, 1 / b and sqrt(b) as the fp64 RRTMG_SW instantiation evaluates them on the device
 * (hardware reciprocal / reciprocal square root + Newton steps + a residual correction: <= 1 ulp for operands in the normal range;
 * tests/test_gpu_fastmath.py). */
int geosrad_dbg_fast64(int n, const double *a, const double *b, double *quot, double *rcp, double *root);

/* Debug / test hooks: gas optical depth and Planck fraction as the reference's taumol leaves them,
 * Fortran (nlay,140,ncol), host pointers; ncol*nlay*140 reals each.  Uses the same kernels as
 * geosrad_rrtmg_lw with an extra store. */
int geosrad_rrtmg_lw_taumol(geosrad_ctx *ctx, int ncol, int nlay,
                            const void *play, const void *plev, const void *tlay, const void *tlev,
                            const void *tsfc, const void *emis,
                            const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr,
                            const void *n2ovmr, const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr,
                            const void *cfc22vmr, const void *ccl4vmr, const void *tauaer,
                            void *taug, void *pfracs);

/* ---- RRTMG_SW ------------------------------------------------------------------------------------------
 * rrtmg_sw (SW/rrtmg_sw_rad.F90:68-124), same argument order without the MAPL handle / RC (the return code is
 * the RC).  Real arrays, element type = real_kind, Fortran layouts:
 *   coszen, alat, asdir, asdif, aldir, aldif (ncol); play, tlay, gases, cld, ciwp, clwp, rei, rel, zm (ncol,nlay);
 *   plev (ncol,nlay+1); tauaer, ssaaer, asmaer (ncol,nlay,14) (read only when iaer == 10, else may be NULL);
 *   swuflx, swdflx, swuflxc, swdflxc (ncol,nlay+1); nirr..uvrf, cot* (ncol); fswband, drband, dfband (ncol,14)
 *   (drband/dfband written only when do_drfband != 0); clearCounts int32 (ncol,4).
 *   scon, adjes: double here, rounded to real_kind like the reference's default-real dummy arguments.
 *   bndscl (14 reals), indsolvar (2 reals) and solcycfrac (1 real): HOST pointers in both variants, NULL = absent optional argument.
 *   isolvar in {-1, 0, 1, 2, 3} (rrtmg_sw_rad.F90:893-1127).  1 = position solcycfrac in [0, 1] of the mean solar cycle AvgCyc11 with
 *   NRLSSI2's adjust_solcyc_amplitudes / interpolate_indices (NRLSSI2.F90:236-332): needs solcycfrac (GEOSRAD_EINPUT otherwise, as the
 *   reference's _FAIL).  The GridComp-level entry point geosrad_sw_driver_rrtmg_dev refuses it like SORADCORE does
 *   (GEOS_SolarGridComp.F90:6286-6292).
 *   rpart (the reference's column-partition size) is accepted and ignored: the GPU batches internally. */
int geosrad_rrtmg_sw(geosrad_ctx *ctx, int rpart, int ncol, int nlay, double scon, double adjes, const void *coszen, int isolvar,
                     const void *play, const void *plev, const void *tlay,
                     const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr,
                     int iceflgsw, int liqflgsw,
                     const void *cld, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                     int dyofyr, const void *zm, const void *alat,
                     int iaer, const void *tauaer, const void *ssaaer, const void *asmaer,
                     const void *asdir, const void *asdif, const void *aldir, const void *aldif,
                     int cloudLM, int cloudMH, int normFlx,
                     int32_t *clearCounts, void *swuflx, void *swdflx, void *swuflxc, void *swdflxc,
                     void *nirr, void *nirf, void *parr, void *parf, void *uvrr, void *uvrf, void *fswband,
                     void *cotdtp, void *cotdhp, void *cotdmp, void *cotdlp,
                     void *cotntp, void *cotnhp, void *cotnmp, void *cotnlp,
                     int do_drfband, void *drband, void *dfband, const void *bndscl, const void *indsolvar,
                     const void *solcycfrac);
/* same, DEVICE pointers, asynchronous on `stream`; input assertions are reported by geosrad_check() */
int geosrad_rrtmg_sw_dev(geosrad_ctx *ctx, void *stream, int rpart, int ncol, int nlay, double scon, double adjes,
                         const void *coszen, int isolvar,
                         const void *play, const void *plev, const void *tlay,
                         const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr,
                         int iceflgsw, int liqflgsw,
                         const void *cld, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                         int dyofyr, const void *zm, const void *alat,
                         int iaer, const void *tauaer, const void *ssaaer, const void *asmaer,
                         const void *asdir, const void *asdif, const void *aldir, const void *aldif,
                         int cloudLM, int cloudMH, int normFlx,
                         int32_t *clearCounts, void *swuflx, void *swdflx, void *swuflxc, void *swdflxc,
                         void *nirr, void *nirf, void *parr, void *parf, void *uvrr, void *uvrf, void *fswband,
                         void *cotdtp, void *cotdhp, void *cotdmp, void *cotdlp,
                         void *cotntp, void *cotnhp, void *cotnmp, void *cotnlp,
                         int do_drfband, void *drband, void *dfband, const void *bndscl, const void *indsolvar,
                         const void *solcycfrac);
/* ---- RRTMG_SW, SOLAR_RADVAL build ----------------------------------------------------------------------
 * rrtmg_sw as the reference compiles it with -DSOLAR_RADVAL (GEOSsolar_GridComp/CMakeLists.txt:18-21): the cloud-optics
 * validation diagnostics of the PAR super-band, the dummy arguments cdsdtp .. forinlp of SW/rrtmg_sw_rad.F90:86-119
 * (declared :300 on), which spcvmc_sw accumulates beside cotd?? / cotn?? (SW/rrtmg_sw_spcvmc.F90:676-746, :749-1109) from the
 * phase-split cloud optics of cldprmc_sw (SW/rrtmg_sw_cldprmc.F90:321-351, :394-410).  15 families, each a denominator `d` and a
 * numerator `n` for the whole column (tp) and the high, middle and low pressure super-layers (hp, mp, lp):
 *   cds            combined liquid + ice, delta-scaled optical thickness (cot?? is its un-scaled twin)
 *   cotl cdsl coti cdsi   optical thickness of the liquid / ice phase, un-scaled (cot) / delta-scaled (cds)
 *   ssal sdsl ssai sdsi   single-scattering albedo                    asml adsl asmi adsi   asymmetry parameter
 *   forl fori             forward-scattering fraction (delta-scaled)
 * The two entry points below are geosrad_rrtmg_sw / geosrad_rrtmg_sw_dev (same arguments, same results for every one of them) plus
 * `radval`: reals (ncol, GEOSRAD_RV_COUNT), column fastest, slot k = the k-th of those dummy arguments in the reference's order
 * (enum below); host pointer for geosrad_rrtmg_sw_radval (it takes the chunked pipeline and the shards of a geosrad_create_multi
 * context like every other output), device pointer for geosrad_rrtmg_sw_radval_dev.  Cloud-free columns get zeros
 * (rrtmg_sw_rad.F90:1540-1590), cloudy ones the sums (:1658-1720).  normFlx does not touch these outputs: the reference divides the
 * fluxes and band fluxes only (:1769-1798).  The 20 PAR sub-columns are summed in the groups in which the band sweeps sum their own
 * cotd?? / cotn?? family (k_sw_reform: its units of g-points; GEOSRAD_SW_PATH=bands: the three bands), not strictly in g-point order: a family
 * that coincides with cot?? (cotl?? of a liquid-only column) then has its bits, and the 120 values may differ in the last bits between the
 * two GEOSRAD_SW_PATH values and from the reference's sequential sum (measured 3.7e-7 relative in fp32).  The sums are formed once per call whatever iaer is (they do not depend on the aerosols);
 * the workspace they need (3.6 KB per column in fp32) is taken at the first such call and reported by geosrad_workspace_bytes. */
enum {
    GEOSRAD_RV_CDSDTP, GEOSRAD_RV_CDSDHP, GEOSRAD_RV_CDSDMP, GEOSRAD_RV_CDSDLP, GEOSRAD_RV_CDSNTP, GEOSRAD_RV_CDSNHP, GEOSRAD_RV_CDSNMP, GEOSRAD_RV_CDSNLP,
    GEOSRAD_RV_COTLDTP, GEOSRAD_RV_COTLDHP, GEOSRAD_RV_COTLDMP, GEOSRAD_RV_COTLDLP, GEOSRAD_RV_COTLNTP, GEOSRAD_RV_COTLNHP, GEOSRAD_RV_COTLNMP, GEOSRAD_RV_COTLNLP,
    GEOSRAD_RV_CDSLDTP, GEOSRAD_RV_CDSLDHP, GEOSRAD_RV_CDSLDMP, GEOSRAD_RV_CDSLDLP, GEOSRAD_RV_CDSLNTP, GEOSRAD_RV_CDSLNHP, GEOSRAD_RV_CDSLNMP, GEOSRAD_RV_CDSLNLP,
    GEOSRAD_RV_COTIDTP, GEOSRAD_RV_COTIDHP, GEOSRAD_RV_COTIDMP, GEOSRAD_RV_COTIDLP, GEOSRAD_RV_COTINTP, GEOSRAD_RV_COTINHP, GEOSRAD_RV_COTINMP, GEOSRAD_RV_COTINLP,
    GEOSRAD_RV_CDSIDTP, GEOSRAD_RV_CDSIDHP, GEOSRAD_RV_CDSIDMP, GEOSRAD_RV_CDSIDLP, GEOSRAD_RV_CDSINTP, GEOSRAD_RV_CDSINHP, GEOSRAD_RV_CDSINMP, GEOSRAD_RV_CDSINLP,
    GEOSRAD_RV_SSALDTP, GEOSRAD_RV_SSALDHP, GEOSRAD_RV_SSALDMP, GEOSRAD_RV_SSALDLP, GEOSRAD_RV_SSALNTP, GEOSRAD_RV_SSALNHP, GEOSRAD_RV_SSALNMP, GEOSRAD_RV_SSALNLP,
    GEOSRAD_RV_SDSLDTP, GEOSRAD_RV_SDSLDHP, GEOSRAD_RV_SDSLDMP, GEOSRAD_RV_SDSLDLP, GEOSRAD_RV_SDSLNTP, GEOSRAD_RV_SDSLNHP, GEOSRAD_RV_SDSLNMP, GEOSRAD_RV_SDSLNLP,
    GEOSRAD_RV_SSAIDTP, GEOSRAD_RV_SSAIDHP, GEOSRAD_RV_SSAIDMP, GEOSRAD_RV_SSAIDLP, GEOSRAD_RV_SSAINTP, GEOSRAD_RV_SSAINHP, GEOSRAD_RV_SSAINMP, GEOSRAD_RV_SSAINLP,
    GEOSRAD_RV_SDSIDTP, GEOSRAD_RV_SDSIDHP, GEOSRAD_RV_SDSIDMP, GEOSRAD_RV_SDSIDLP, GEOSRAD_RV_SDSINTP, GEOSRAD_RV_SDSINHP, GEOSRAD_RV_SDSINMP, GEOSRAD_RV_SDSINLP,
    GEOSRAD_RV_ASMLDTP, GEOSRAD_RV_ASMLDHP, GEOSRAD_RV_ASMLDMP, GEOSRAD_RV_ASMLDLP, GEOSRAD_RV_ASMLNTP, GEOSRAD_RV_ASMLNHP, GEOSRAD_RV_ASMLNMP, GEOSRAD_RV_ASMLNLP,
    GEOSRAD_RV_ADSLDTP, GEOSRAD_RV_ADSLDHP, GEOSRAD_RV_ADSLDMP, GEOSRAD_RV_ADSLDLP, GEOSRAD_RV_ADSLNTP, GEOSRAD_RV_ADSLNHP, GEOSRAD_RV_ADSLNMP, GEOSRAD_RV_ADSLNLP,
    GEOSRAD_RV_ASMIDTP, GEOSRAD_RV_ASMIDHP, GEOSRAD_RV_ASMIDMP, GEOSRAD_RV_ASMIDLP, GEOSRAD_RV_ASMINTP, GEOSRAD_RV_ASMINHP, GEOSRAD_RV_ASMINMP, GEOSRAD_RV_ASMINLP,
    GEOSRAD_RV_ADSIDTP, GEOSRAD_RV_ADSIDHP, GEOSRAD_RV_ADSIDMP, GEOSRAD_RV_ADSIDLP, GEOSRAD_RV_ADSINTP, GEOSRAD_RV_ADSINHP, GEOSRAD_RV_ADSINMP, GEOSRAD_RV_ADSINLP,
    GEOSRAD_RV_FORLDTP, GEOSRAD_RV_FORLDHP, GEOSRAD_RV_FORLDMP, GEOSRAD_RV_FORLDLP, GEOSRAD_RV_FORLNTP, GEOSRAD_RV_FORLNHP, GEOSRAD_RV_FORLNMP, GEOSRAD_RV_FORLNLP,
    GEOSRAD_RV_FORIDTP, GEOSRAD_RV_FORIDHP, GEOSRAD_RV_FORIDMP, GEOSRAD_RV_FORIDLP, GEOSRAD_RV_FORINTP, GEOSRAD_RV_FORINHP, GEOSRAD_RV_FORINMP, GEOSRAD_RV_FORINLP,
    GEOSRAD_RV_COUNT
};
int geosrad_rrtmg_sw_radval(geosrad_ctx *ctx, int rpart, int ncol, int nlay, double scon, double adjes,
                            const void *coszen, int isolvar,
                            const void *play, const void *plev, const void *tlay,
                            const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr,
                            int iceflgsw, int liqflgsw,
                            const void *cld, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                            int dyofyr, const void *zm, const void *alat,
                            int iaer, const void *tauaer, const void *ssaaer, const void *asmaer,
                            const void *asdir, const void *asdif, const void *aldir, const void *aldif,
                            int cloudLM, int cloudMH, int normFlx,
                            int32_t *clearCounts, void *swuflx, void *swdflx, void *swuflxc, void *swdflxc,
                            void *nirr, void *nirf, void *parr, void *parf, void *uvrr, void *uvrf, void *fswband,
                            void *cotdtp, void *cotdhp, void *cotdmp, void *cotdlp,
                            void *cotntp, void *cotnhp, void *cotnmp, void *cotnlp,
                            int do_drfband, void *drband, void *dfband, const void *bndscl, const void *indsolvar,
                            const void *solcycfrac, void *radval);
/* same, DEVICE pointers (radval included), asynchronous on `stream` */
int geosrad_rrtmg_sw_radval_dev(geosrad_ctx *ctx, void *stream, int rpart, int ncol, int nlay, double scon, double adjes,
                                const void *coszen, int isolvar,
                                const void *play, const void *plev, const void *tlay,
                                const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr,
                                int iceflgsw, int liqflgsw,
                                const void *cld, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                                int dyofyr, const void *zm, const void *alat,
                                int iaer, const void *tauaer, const void *ssaaer, const void *asmaer,
                                const void *asdir, const void *asdif, const void *aldir, const void *aldif,
                                int cloudLM, int cloudMH, int normFlx,
                                int32_t *clearCounts, void *swuflx, void *swdflx, void *swuflxc, void *swdflxc,
                                void *nirr, void *nirf, void *parr, void *parf, void *uvrr, void *uvrf, void *fswband,
                                void *cotdtp, void *cotdhp, void *cotdmp, void *cotdlp,
                                void *cotntp, void *cotnhp, void *cotnmp, void *cotnlp,
                                int do_drfband, void *drband, void *dfband, const void *bndscl, const void *indsolvar,
                                const void *solcycfrac, void *radval);
/* Debug / test hook: taug, taur Fortran (nlay,112,ncol) and the solar source ssi (112,ncol) [sfluxzen when
 * isolvar < 0] as the reference's taumol_sw leaves them (SW/rrtmg_sw_taumol.F90:27); host pointers. */
int geosrad_rrtmg_sw_taumol(geosrad_ctx *ctx, int ncol, int nlay, double scon, int isolvar,
                            const void *play, const void *plev, const void *tlay,
                            const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr,
                            const void *bndscl, const void *indsolvar, const void *solcycfrac,
                            void *taug, void *taur, void *ssi);
/* Debug / test hook: the McICA cloud optics of the solver's own sub-columns - delta-scaled optical depth, single-scattering
 * albedo and asymmetry parameter, Fortran (nlay,112,ncol), as the reference's cldprmc_sw leaves taucmc, ssacmc, asmcmc
 * (SW/rrtmg_sw_cldprmc.F90:36-418; 0, 1, 0 in clear cells); host pointers. */
int geosrad_rrtmg_sw_cldprmc(geosrad_ctx *ctx, int ncol, int nlay, const void *play, const void *plev, const void *tlay,
                             const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *o2vmr,
                             int iceflgsw, int liqflgsw, const void *cld, const void *ciwp, const void *clwp, const void *rei,
                             const void *rel, int dyofyr, const void *zm, const void *alat, int cloudLM, int cloudMH,
                             void *taucmc, void *ssacmc, void *asmcmc);

/* ---- Chou-Suarez longwave ------------------------------------------------------------------------------
 * irrad (GEOSirrad_GridComp/irrad.F90:27-35), same argument order (the logical `trace` as int).  Layers from the TOP down
 * (k = 1 top layer), ple in Pa; Fortran layouts: ple (m,np+1); ta, wa, oa, n2o, ch4, cfc11, cfc12, cfc22, fcld (m,np); tb (m);
 * cwc, reff (m,np,4); fs, tg, tv (m,ns); eg, ev, rv (m,ns,10); taua, ssaa, asya (m,np,nb) are IN-OUT and rescaled in place
 * exactly like the reference does (irrad.F90:655-678; may be NULL when na == 0); outputs flxu ... flxad, dfdts (m,np+1),
 * sfcem (m), taudiag (m,np,10).  Upward fluxes are negative.  Maximum-random overlap, or the -DOVERCAST behaviour under
 * GEOSRAD_OVERCAST_IRRAD (geosrad_set_overcast; ict / icb are then not read).
 * trace == 0: band 10 is skipped for every column (the reference `return`s out of its column loop there, irrad.F90:478;
 * GEOS always passes trace = .true.). */
int geosrad_irrad(geosrad_ctx *ctx, int m, int np, const void *ple, const void *ta, const void *wa, const void *oa, const void *tb,
                  double co2, int trace, const void *n2o, const void *ch4, const void *cfc11, const void *cfc12, const void *cfc22,
                  const void *cwc, const void *fcld, int ict, int icb, const void *reff,
                  int ns, const void *fs, const void *tg, const void *eg, const void *tv, const void *ev, const void *rv,
                  int na, int nb, void *taua, void *ssaa, void *asya,
                  void *flxu, void *flcu, void *flau, void *flxau, void *flxd, void *flcd, void *flad, void *flxad,
                  void *dfdts, void *sfcem, void *taudiag);
int geosrad_irrad_dev(geosrad_ctx *ctx, void *stream, int m, int np, const void *ple, const void *ta, const void *wa, const void *oa,
                      const void *tb, double co2, int trace, const void *n2o, const void *ch4, const void *cfc11, const void *cfc12,
                      const void *cfc22, const void *cwc, const void *fcld, int ict, int icb, const void *reff,
                      int ns, const void *fs, const void *tg, const void *eg, const void *tv, const void *ev, const void *rv,
                      int na, int nb, void *taua, void *ssaa, void *asya,
                      void *flxu, void *flcu, void *flau, void *flxau, void *flxd, void *flcd, void *flad, void *flxad,
                      void *dfdts, void *sfcem, void *taudiag);

/* ---- Chou-Suarez shortwave -----------------------------------------------------------------------------
 * sorad (GEOSsolar_GridComp/sorad.F90:43-51), same argument order.  Layers from the TOP down, pl in hPa; Fortran layouts:
 * cosz, rsuvbm, rsuvdf, rsirbm, rsirdf (m); pl (m,np+1); ta, wa, oa, fcld (m,np); cwc, reff (m,np,4); taua, ssaa, asya
 * (m,np,nb = 8) in the (tau, tau*ssa, tau*ssa*g) form the reference expects; hk_uv (5), hk_ir (3,10): HOST pointers in both
 * variants; outputs flx, flc, flxu, flcu (m,np+1), fdir/fdif uv/par/ir (m), flx_sfc_band (m,8), drband, dfband (m,8; written
 * only when do_drfband != 0, else may be NULL).  Fluxes are fractions of the TOA insolation.  Maximum-random overlap, or the -DOVERCAST
 * behaviour under GEOSRAD_OVERCAST_SORAD (geosrad_set_overcast; ict / icb are then not read). */
int geosrad_sorad(geosrad_ctx *ctx, int m, int np, int nb, const void *cosz, const void *pl, const void *ta, const void *wa,
                  const void *oa, double co2, const void *cwc, const void *fcld, int ict, int icb, const void *reff,
                  const void *hk_uv, const void *hk_ir, const void *taua, const void *ssaa, const void *asya,
                  const void *rsuvbm, const void *rsuvdf, const void *rsirbm, const void *rsirdf,
                  void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar, void *fdifpar, void *fdirir, void *fdifir,
                  void *flxu, void *flcu, void *flx_sfc_band, int do_drfband, void *drband, void *dfband);
int geosrad_sorad_dev(geosrad_ctx *ctx, void *stream, int m, int np, int nb, const void *cosz, const void *pl, const void *ta,
                      const void *wa, const void *oa, double co2, const void *cwc, const void *fcld, int ict, int icb,
                      const void *reff, const void *hk_uv, const void *hk_ir, const void *taua, const void *ssaa, const void *asya,
                      const void *rsuvbm, const void *rsuvdf, const void *rsirbm, const void *rsirdf,
                      void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar, void *fdifpar, void *fdirir, void *fdifir,
                      void *flxu, void *flcu, void *flx_sfc_band, int do_drfband, void *drband, void *dfband);

/* geosrad_sorad_na / geosrad_sorad_na_dev: geosrad_sorad / geosrad_sorad_dev (the same arguments in the same order) + the aerosol-free
 * fluxes of the same columns from the same call.  The Solar GridComp obtains its aerosol-free internals FSWNAN, FSCNAN, FSWUNAN, FSCUNAN,
 * FSWBANDNAN by running the whole of SORADCORE a second time with include_aerosols = .false. (GEOS_SolarGridComp.F90:3249-3259 the second
 * call, :3997-4016 the internals it fills - never DRBANDN / DFBANDN -, :4541-4551 the zero aerosol arrays the Chou-Suarez branch then hands
 * sorad).  Here the preparation (classes, partition, absorber amounts, cloud optics) runs once, and after the with-aerosol spectral
 * passes, sum and reduction the 35 passes run once more with no aerosol (nothing is read from taua / ssaa / asya), followed by their own
 * sum and reduction.
 *   na_out: HOST array of GEOSRAD_SONA_NOUT pointers (host arrays for geosrad_sorad_na, device arrays for geosrad_sorad_na_dev), indexed
 *   by GEOSRAD_SONA_*: the twins of flx, flc, flxu, flcu (m,np+1) and of flx_sfc_band (m,8).  Each is bit for bit what geosrad_sorad[_dev]
 *   returns in its twin for the same columns with three aerosol arrays of zeros.  Any member may be NULL: it is left untouched.  na_out
 *   NULL, or all its members NULL: the plain call, no second pass runs.
 * The 13 regular outputs are bit for bit those of geosrad_sorad[_dev]; the aerosol-free pass has no direct / diffuse components and no
 * drband / dfband (do_drfband keeps its meaning for the with-aerosol pass).  The workspace is that of the plain call (the second pass reuses
 * it) plus the place of every member of na_out that is NULL.  Errors as geosrad_sorad[_dev], nothing launched. */
enum { GEOSRAD_SONA_FLX, GEOSRAD_SONA_FLC, GEOSRAD_SONA_FLXU, GEOSRAD_SONA_FLCU, GEOSRAD_SONA_SFCBAND /*(m,8)*/, GEOSRAD_SONA_NOUT };
int geosrad_sorad_na(geosrad_ctx *ctx, int m, int np, int nb, const void *cosz, const void *pl, const void *ta, const void *wa,
                     const void *oa, double co2, const void *cwc, const void *fcld, int ict, int icb, const void *reff,
                     const void *hk_uv, const void *hk_ir, const void *taua, const void *ssaa, const void *asya,
                     const void *rsuvbm, const void *rsuvdf, const void *rsirbm, const void *rsirdf,
                     void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar, void *fdifpar, void *fdirir, void *fdifir,
                     void *flxu, void *flcu, void *flx_sfc_band, int do_drfband, void *drband, void *dfband, void *const *na_out);
int geosrad_sorad_na_dev(geosrad_ctx *ctx, void *stream, int m, int np, int nb, const void *cosz, const void *pl, const void *ta,
                         const void *wa, const void *oa, double co2, const void *cwc, const void *fcld, int ict, int icb,
                         const void *reff, const void *hk_uv, const void *hk_ir, const void *taua, const void *ssaa, const void *asya,
                         const void *rsuvbm, const void *rsuvdf, const void *rsirbm, const void *rsirdf,
                         void *flx, void *flc, void *fdiruv, void *fdifuv, void *fdirpar, void *fdifpar, void *fdirir, void *fdifir,
                         void *flxu, void *flcu, void *flx_sfc_band, int do_drfband, void *drband, void *dfband, void *const *na_out);

/* ---- McICA ------------------------------------------------------------------------------------------
 * generate_stochastic_clouds (cloud_subcol_gen.F90:132): profile inputs Fortran (nlay,dncol) there; here
 * the solver-API layout (ncol,nlay) is used for the inputs (what rrtmg_lw receives), outputs are
 * Fortran (nlay,nsubcol,ncol): cldy int32 (0/1), ciwp_stoch, clwp_stoch reals. */
int geosrad_mcica(geosrad_ctx *ctx, int ncol, int nsubcol, int nlay,
                  const void *zmid, const void *alat, int doy, const void *play, const void *cldfrac,
                  const void *ciwp, const void *clwp, double cwp_tiny, const int32_t seed_order[4],
                  int32_t *cldy_stoch, void *ciwp_stoch, void *clwp_stoch);
/* same, DEVICE pointers, asynchronous on `stream` (seed_order stays a host pointer) */
int geosrad_mcica_dev(geosrad_ctx *ctx, void *stream, int ncol, int nsubcol, int nlay,
                      const void *zmid, const void *alat, int doy, const void *play, const void *cldfrac,
                      const void *ciwp, const void *clwp, double cwp_tiny, const int32_t seed_order[4],
                      int32_t *cldy_stoch, void *ciwp_stoch, void *clwp_stoch);
/* clearCounts_threeBand (cloud_subcol_gen.F90:611): cldy (nlay,nsubcol,ncol) int32 -> clearCnts (4,ncol) */
int geosrad_clearcounts(geosrad_ctx *ctx, int ncol, int nsubcol, int nlay, int cloudLM, int cloudMH,
                        const int32_t *cldy_stoch, int32_t *clearCnts);

/* ---- RATS diagnostics (GEOS_IrradGridComp.F90:3389-3469) ------------------------------------------
 * LW_Driver calls rrtmg_lw once more per gas listed under RATS_DIAGNOSTICS: with that gas's mixing ratio set to zero and keeps
 * the total-sky UFLX, DFLX, DUFLX_DTS of each call.  geosrad_rrtmg_lw_rats_dev = geosrad_rrtmg_lw_dev (same arguments, same
 * results) + those profiles for `nrats` gases from the SAME call: uflx_rat, dflx_rat, duflx_dTs_rat are (ncol,nlay+1,nrats)
 * device arrays (gas slowest, like UFLXRAT(IM*JM,LM+1,nRATS), :3390-3392).  The input checks, the clear | cloudy partition, the
 * overlap correlations, the McICA sub-columns with their cloud optical depths and clearCounts do not depend on the gases and are
 * computed once; a gas costs setcoef + the band sweeps + the flux reduction.  Results are bitwise those of a separate call with the
 * gas's array zeroed.  NB the reference zeroes HCFC22 under the name 'HCFC22_R' but restores it under 'HCFC22' (:3434, :3464), so
 * that toggle never matches there; GEOSRAD_RAT_HCFC22 implements the evident intent. */
enum { GEOSRAD_RAT_H2O, GEOSRAD_RAT_O3, GEOSRAD_RAT_CO2, GEOSRAD_RAT_CH4, GEOSRAD_RAT_N2O, GEOSRAD_RAT_CFC11, GEOSRAD_RAT_CFC12,
       GEOSRAD_RAT_HCFC22, GEOSRAD_RAT_NGAS };
int geosrad_rrtmg_lw_rats_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlay, int psize, int dudTs,
                              const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc, const void *emis,
                              const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
                              const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr, const void *ccl4vmr,
                              const void *cldf, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                              int iceflglw, int liqflglw, const void *tauaer, const void *zm, const void *alat, int dyofyr,
                              int cloudLM, int cloudMH, int32_t *clearCounts,
                              void *uflx, void *dflx, void *uflxc, void *dflxc, void *duflx_dTs, void *duflxc_dTs,
                              const int32_t *band_output, void *olrb, void *dolrb_dTs,
                              int nrats, const int32_t *rat_gas /*host, GEOSRAD_RAT_**/, void *uflx_rat, void *dflx_rat,
                              void *duflx_dTs_rat);

/* ---- Aerosol-free RRTMG_LW fluxes -------------------------------------------------------------------------------------------
 * The INTERNALs FLXAU / FLXAD / FLAU / FLAD (total-sky and clear-sky fluxes without aerosols) are filled by the reference's
 * Chou-Suarez branch (inside irrad) and by its RRTMGP branch (calc_clrnoa); its RRTMG branch leaves their exports MAPL_UNDEF and copies
 * DFDTSNA = DFDTS (GEOS_IrradGridComp.F90:3552-3556, :3927-3990).  geosrad_rrtmg_lw_na_dev = geosrad_rrtmg_lw_rats_dev (same
 * arguments, nrats may be 0) + the six flux arrays of the same columns with tauaer taken away, from the SAME call: uflx_na, dflx_na,
 * uflxc_na, dflxc_na, duflx_dTs_na, duflxc_dTs_na are (ncol,nlay+1); the first four are required, the two derivatives are required iff
 * dudTs and ignored otherwise.  Nothing the clouds decide depends on the aerosols (the partition, the overlap, the sub-columns with their
 * optical depths, clearCounts), and neither does setcoef: the aerosol-free fluxes cost one more band sweep and one more reduction.  They
 * are bitwise those of a separate call with tauaer == NULL.  With tauaer == NULL there is nothing to remove: no second sweep runs and the
 * six arrays receive the bits of uflx .. duflxc_dTs.
 * Like a call with RATS diagnostics, such a call takes the band-partials path THROUGHOUT, its main pass included (the passes share the
 * per-band partials of the reduction): under GEOSRAD_LW_PATH=cols its with-aerosol outputs have the bits of geosrad_rrtmg_lw_rats_dev,
 * not those of geosrad_rrtmg_lw_dev.  It holds the second set of partials also with nrats == 0 (geosrad_workspace_bytes counts it) and
 * honours geosrad_set_chunk; results do not depend on the chunk size.
 * geosrad_rrtmg_lw_na: geosrad_rrtmg_lw (host pointers, chunked pipeline, sharded by a geosrad_create_multi context) + the same six. */
int geosrad_rrtmg_lw_na_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlay, int psize, int dudTs,
                            const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc, const void *emis,
                            const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
                            const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr, const void *ccl4vmr,
                            const void *cldf, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                            int iceflglw, int liqflglw, const void *tauaer, const void *zm, const void *alat, int dyofyr,
                            int cloudLM, int cloudMH, int32_t *clearCounts,
                            void *uflx, void *dflx, void *uflxc, void *dflxc, void *duflx_dTs, void *duflxc_dTs,
                            const int32_t *band_output, void *olrb, void *dolrb_dTs,
                            int nrats, const int32_t *rat_gas /*host, GEOSRAD_RAT_**/, void *uflx_rat, void *dflx_rat,
                            void *duflx_dTs_rat,
                            void *uflx_na, void *dflx_na, void *uflxc_na, void *dflxc_na, void *duflx_dTs_na, void *duflxc_dTs_na);
int geosrad_rrtmg_lw_na(geosrad_ctx *ctx, int ncol, int nlay, int psize, int dudTs,
                        const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc, const void *emis,
                        const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
                        const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr, const void *ccl4vmr,
                        const void *cldf, const void *ciwp, const void *clwp, const void *rei, const void *rel,
                        int iceflglw, int liqflglw, const void *tauaer, const void *zm, const void *alat, int dyofyr,
                        int cloudLM, int cloudMH, int32_t *clearCounts,
                        void *uflx, void *dflx, void *uflxc, void *dflxc, void *duflx_dTs, void *duflxc_dTs,
                        const int32_t *band_output, void *olrb, void *dolrb_dTs,
                        void *uflx_na, void *dflx_na, void *uflxc_na, void *dflxc_na, void *duflx_dTs_na, void *duflxc_dTs_na);

/* ---- GridComp data path either side of the solvers -------------------------------------
 * All arrays are DEVICE pointers of the context's real kind in the GEOS layout (IM*JM columns fastest, then the level /
 * layer index in MODEL ordering, 1 = top), asynchronous on `stream`.  A NULL output = Fortran "not associated" (export
 * not requested).  MAPL's physical constants are not defined in the reference repository: the caller passes them.
 *
 * geosrad_lw_driver_rrtmg_dev: the RRTMG branch of LW_Driver (GEOS_IrradGridComp.F90:3188-3372 prep / flip, :3470-3477 the
 * rrtmg_lw call with Ts_derivs = .true., :3487-3533 + :3560-3565 + :3601-3615 un-flip, sign conventions, SFCEM, net fluxes).
 * lcldlm / lcldmh are the MODEL-ordering super-layer interface indices (the routine flips them like IRR:3237-3239). */
enum { GEOSRAD_LWD_PLE /*(ncol,0:LM) Pa*/, GEOSRAD_LWD_PL /*(ncol,LM) Pa*/, GEOSRAD_LWD_T, GEOSRAD_LWD_Q, GEOSRAD_LWD_O3,
       GEOSRAD_LWD_CH4, GEOSRAD_LWD_N2O, GEOSRAD_LWD_CO2_3D /*nullable: CO2_FIXED is used*/, GEOSRAD_LWD_CFC11, GEOSRAD_LWD_CFC12,
       GEOSRAD_LWD_HCFC22, GEOSRAD_LWD_FCLD, GEOSRAD_LWD_CWC_LIQ, GEOSRAD_LWD_CWC_ICE, GEOSRAD_LWD_REFF_LIQ, GEOSRAD_LWD_REFF_ICE,
       GEOSRAD_LWD_TAUA /*(ncol,LM,nb) nullable*/, GEOSRAD_LWD_SSAA, GEOSRAD_LWD_TS /*(ncol)*/, GEOSRAD_LWD_EMIS, GEOSRAD_LWD_LATS,
       GEOSRAD_LWD_T2M, GEOSRAD_LWD_NIN };
enum { GEOSRAD_LWD_C_CO2_FIXED, GEOSRAD_LWD_C_O2, GEOSRAD_LWD_C_CCL4, GEOSRAD_C_AIRMW, GEOSRAD_C_H2OMW, GEOSRAD_C_O3MW,
       GEOSRAD_C_RGAS, GEOSRAD_C_GRAV, GEOSRAD_LWD_NCONST };
enum { GEOSRAD_LWD_FLXU_INT /*(ncol,0:LM)*/, GEOSRAD_LWD_FLXD_INT, GEOSRAD_LWD_FLCU_INT, GEOSRAD_LWD_FLCD_INT, GEOSRAD_LWD_DFDTS,
       GEOSRAD_LWD_DFDTSC, GEOSRAD_LWD_DFDTSNA, GEOSRAD_LWD_DFDTSCNA, GEOSRAD_LWD_FLX_INT, GEOSRAD_LWD_FLC_INT,
       GEOSRAD_LWD_SFCEM_INT /*(ncol), positive*/, GEOSRAD_LWD_TS_INT, GEOSRAD_LWD_CLDTTLW, GEOSRAD_LWD_CLDHILW, GEOSRAD_LWD_CLDMDLW,
       GEOSRAD_LWD_CLDLOLW, GEOSRAD_LWD_OLRB /*(16,ncol)*/, GEOSRAD_LWD_DOLRB, GEOSRAD_LWD_NOUT };
int geosrad_lw_driver_rrtmg_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int nb_aer, const void *const *in,
                                const double *consts, int iceflglw, int liqflglw, int doy, int lcldlm, int lcldmh,
                                const int32_t *band_output, void *const *out);
/* the same with the RATS loop (GEOS_IrradGridComp.F90:3389-3469) and its share of the un-flip (:3522-3530, :3614): rat_out =
 * INTERNAL FLXU_RAT, FLXD_RAT, FLX_RAT, DFDTS_RAT (ncol,0:LM,nrats) and SFCEM_RAT (ncol,nrats); any may be NULL. */
enum { GEOSRAD_LWD_FLXU_RAT, GEOSRAD_LWD_FLXD_RAT, GEOSRAD_LWD_FLX_RAT, GEOSRAD_LWD_DFDTS_RAT, GEOSRAD_LWD_SFCEM_RAT, GEOSRAD_LWD_NRATOUT };
int geosrad_lw_driver_rrtmg_rats_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int nb_aer, const void *const *in,
                                     const double *consts, int iceflglw, int liqflglw, int doy, int lcldlm, int lcldmh,
                                     const int32_t *band_output, void *const *out, int nrats, const int32_t *rat_gas,
                                     void *const *rat_out);
/* the same with the aerosol-free INTERNALs from geosrad_rrtmg_lw_na_dev (nrats may be 0): na_out = FLXAU_INT, FLXAD_INT, FLAU_INT,
 * FLAD_INT, FLXA_INT, FLA_INT, DFDTSNA, DFDTSCNA (ncol,0:LM) in model ordering, with the conventions of GEOS_IrradGridComp.F90:3506-3515
 * and :3604-3607: FLXAU = -uflx_na, FLXAD = dflx_na, FLAU = -uflxc_na, FLAD = dflxc_na, FLXA = FLXAD + FLXAU, FLA = FLAD + FLAU,
 * DFDTSNA = -duflx_dTs_na, DFDTSCNA = -duflxc_dTs_na - the derivatives of the aerosol-free pass itself.  Any may be NULL; with all eight
 * NULL, or na_out NULL, the call is geosrad_lw_driver_rrtmg_rats_dev and no second sweep runs.  out[GEOSRAD_LWD_DFDTSNA / _DFDTSCNA] keep
 * the reference's meaning (copies of DFDTS / DFDTSC, :3560-3565): a caller who wants the real ones in its INTERNAL state passes NULL there
 * and the field here.  (Without TAUA / SSAA the solver is handed an all-zero tauaer, as by the other two drivers, and sweeps it twice for
 * equal results.)  An RRTMG caller who has filled these INTERNALs calls geosrad_lw_update_flx_dev with rrtmg = 0, which reads them as real
 * fields, and GEOSRAD_RT_FLA of geosrad_rad_tendencies_dev then yields RADLWCNA. */
enum { GEOSRAD_LWNA_FLXAU_INT, GEOSRAD_LWNA_FLXAD_INT, GEOSRAD_LWNA_FLAU_INT, GEOSRAD_LWNA_FLAD_INT, GEOSRAD_LWNA_FLXA_INT,
       GEOSRAD_LWNA_FLA_INT, GEOSRAD_LWNA_DFDTSNA, GEOSRAD_LWNA_DFDTSCNA, GEOSRAD_LWNA_NOUT };
int geosrad_lw_driver_rrtmg_na_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int nb_aer, const void *const *in,
                                   const double *consts, int iceflglw, int liqflglw, int doy, int lcldlm, int lcldmh,
                                   const int32_t *band_output, void *const *out, int nrats, const int32_t *rat_gas,
                                   void *const *rat_out, void *const *na_out);

/* geosrad_lw_chou_post_dev: what the Chou-Suarez branch of LW_Driver adds after `call IRRAD` (which takes the GEOS fields as they are):
 * DFDTSC = 0, DFDTSNA = DFDTS, DFDTSCNA = 0 (GEOS_IrradGridComp.F90:2101-2108), the four net fluxes FL*_INT = FL*D_INT + FL*U_INT,
 * SFCEM_INT = -SFCEM_INT (in place), TS_INT = TS (:3601-3616).  Outputs may be NULL. */
enum { GEOSRAD_LWC_FLXU_INT, GEOSRAD_LWC_FLCU_INT, GEOSRAD_LWC_FLAU_INT, GEOSRAD_LWC_FLXAU_INT, GEOSRAD_LWC_FLXD_INT, GEOSRAD_LWC_FLCD_INT,
       GEOSRAD_LWC_FLAD_INT, GEOSRAD_LWC_FLXAD_INT, GEOSRAD_LWC_DFDTS, GEOSRAD_LWC_TS, GEOSRAD_LWC_NIN };
enum { GEOSRAD_LWC_SFCEM_INT /*in-out*/, GEOSRAD_LWC_FLX_INT, GEOSRAD_LWC_FLXA_INT, GEOSRAD_LWC_FLC_INT, GEOSRAD_LWC_FLA_INT, GEOSRAD_LWC_DFDTSC,
       GEOSRAD_LWC_DFDTSNA, GEOSRAD_LWC_DFDTSCNA, GEOSRAD_LWC_TS_INT, GEOSRAD_LWC_NOUT };
int geosrad_lw_chou_post_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, const void *const *in, void *const *out);

/* geosrad_lw_driver_chou_dev: the whole Chou-Suarez branch of LW_Driver in one call (GEOS_IrradGridComp.F90:1781-1785 the FCLD copy with
 * the RADLW_BINARY_CLOUDS option, :1876-1912 T2M, the surface arguments FS / TG / EG / TV / EV / RV with NS = 1, CWC and REFF from the four
 * species with MAPL_UNDEF radii replaced by 36 / 14 / 50 / 50 microns and metres turned into microns, :1966-1970 NA = 0 without aerosols,
 * :2093-2108 `call IRRAD` and the derivatives it does not provide, :3604-3619 net fluxes, the sign of SFCEM, TS_INT, :3626-3650 the infrared
 * cloud exports, :3654-3663 the refresh-time exports).  Fields in the GEOS layout and MODEL ordering (what irrad expects).
 *   in : PLE (ncol,0:LM) Pa; T .. RS (ncol,LM), radii in metres, MAPL_UNDEF allowed; TS, EMIS (ncol); TAUA, SSAA, ASYA (ncol,LM,10) in
 *        irrad's (tau, tau*ssa, tau*ssa*g) form, all three or none (none: NA = 0).  The three aerosol arrays are IN-OUT: rescaled in place
 *        like irrad does (irrad.F90:655-678).  Nothing else is written: unlike the reference's `WHERE (RI == MAPL_UNDEF) RI = 36.e-6`
 *        the imports stay as they are, and FCLD is not changed by binary_clouds.
 *   consts: CO2_FIXED, MAPL_KAPPA, MAPL_UNDEF, TAUCRIT (the resource value, default 0.30; divided by 2.13 in the real kind, :3628).
 *   trace, lcldmh, lcldlm: irrad's TRACE (.true. in the reference, :1487), ict, icb; 1 < lcldmh < lcldlm <= lm (:1917-1943), else
 *        GEOSRAD_EINVAL.  The -DOVERCAST mode of the context (geosrad_set_overcast) applies as for geosrad_irrad_dev.
 *   out: required FLXU_INT .. FLXAD_INT, DFDTS (ncol,0:LM) and SFCEM_INT (ncol), positive on return (:3611).  Optional (NULL = not
 *        associated): FLX_INT, FLXA_INT, FLC_INT, FLA_INT, DFDTSC (= 0), DFDTSNA (= DFDTS), DFDTSCNA (= 0) (ncol,0:LM), TS_INT (ncol);
 *        TAUIR (ncol,LM) = 0.5 (TAUDIAG(3) + TAUDIAG(4)); CLDTMP, CLDPRS (ncol) = T(L), PLE(L-1) of the first layer L from the top with
 *        TAUIR(L) > TAUCRIT / 2.13, MAPL_UNDEF where there is none; TSREFF = TS, DSFDTS0 = -DFDTS(LM), SFCEM0 = SFCEM_INT, LWS0 =
 *        FLX_INT(LM) + SFCEM_INT (needs FLX_INT, else GEOSRAD_EINVAL); and for parity tests T2M (ncol) and irrad's TAUDIAG (ncol,LM,10).
 * Honours geosrad_set_chunk; results do not depend on the chunk size. */
enum { GEOSRAD_LWK_PLE, GEOSRAD_LWK_T, GEOSRAD_LWK_Q, GEOSRAD_LWK_O3, GEOSRAD_LWK_CH4, GEOSRAD_LWK_N2O, GEOSRAD_LWK_CFC11, GEOSRAD_LWK_CFC12,
       GEOSRAD_LWK_HCFC22, GEOSRAD_LWK_FCLD, GEOSRAD_LWK_QI, GEOSRAD_LWK_QL, GEOSRAD_LWK_QR, GEOSRAD_LWK_QS, GEOSRAD_LWK_RI, GEOSRAD_LWK_RL,
       GEOSRAD_LWK_RR, GEOSRAD_LWK_RS, GEOSRAD_LWK_TS, GEOSRAD_LWK_EMIS, GEOSRAD_LWK_TAUA /*in-out, nullable*/, GEOSRAD_LWK_SSAA,
       GEOSRAD_LWK_ASYA, GEOSRAD_LWK_NIN };
enum { GEOSRAD_LWK_C_CO2_FIXED, GEOSRAD_LWK_C_KAPPA, GEOSRAD_LWK_C_UNDEF, GEOSRAD_LWK_C_TAUCRIT, GEOSRAD_LWK_NCONST };
enum { GEOSRAD_LWK_FLXU_INT, GEOSRAD_LWK_FLCU_INT, GEOSRAD_LWK_FLAU_INT, GEOSRAD_LWK_FLXAU_INT, GEOSRAD_LWK_FLXD_INT, GEOSRAD_LWK_FLCD_INT,
       GEOSRAD_LWK_FLAD_INT, GEOSRAD_LWK_FLXAD_INT, GEOSRAD_LWK_DFDTS, GEOSRAD_LWK_SFCEM_INT, GEOSRAD_LWK_FLX_INT, GEOSRAD_LWK_FLXA_INT,
       GEOSRAD_LWK_FLC_INT, GEOSRAD_LWK_FLA_INT, GEOSRAD_LWK_DFDTSC, GEOSRAD_LWK_DFDTSNA, GEOSRAD_LWK_DFDTSCNA, GEOSRAD_LWK_TS_INT,
       GEOSRAD_LWK_TAUIR, GEOSRAD_LWK_CLDTMP, GEOSRAD_LWK_CLDPRS, GEOSRAD_LWK_TSREFF, GEOSRAD_LWK_DSFDTS0, GEOSRAD_LWK_SFCEM0, GEOSRAD_LWK_LWS0,
       GEOSRAD_LWK_T2M, GEOSRAD_LWK_TAUDIAG, GEOSRAD_LWK_NOUT };
int geosrad_lw_driver_chou_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, const void *const *in, const double *consts, int trace,
                               int lcldmh, int lcldlm, int binary_clouds, void *const *out);

/* geosrad_sw_driver_rrtmg_dev: the RRTMG branch of SORADCORE on the packed daytime columns (GEOS_SolarGridComp.F90:6113-6219
 * prep / flip incl. the in-place aerosol normalisation, :6330-6388 the rrtmg_sw call, :6395-6450 un-flip, cloud fractions,
 * in-cloud optical thickness, net fluxes).  ple is (ncol,LM+1).  solvar = {bndscl[14], indsolvar[2]} host pointers or NULL. */
enum { GEOSRAD_SWD_PLE, GEOSRAD_SWD_PL, GEOSRAD_SWD_T, GEOSRAD_SWD_Q, GEOSRAD_SWD_O3, GEOSRAD_SWD_CH4, GEOSRAD_SWD_CL,
       GEOSRAD_SWD_TS, GEOSRAD_SWD_QQ_ICE, GEOSRAD_SWD_QQ_LIQ, GEOSRAD_SWD_RR_ICE, GEOSRAD_SWD_RR_LIQ,
       GEOSRAD_SWD_TAUA /*(ncol,LM,nb) in/out, nullable*/, GEOSRAD_SWD_SSAA, GEOSRAD_SWD_ASYA, GEOSRAD_SWD_ZT /*cos zenith*/,
       GEOSRAD_SWD_ALAT, GEOSRAD_SWD_ALBVR, GEOSRAD_SWD_ALBVF, GEOSRAD_SWD_ALBNR, GEOSRAD_SWD_ALBNF, GEOSRAD_SWD_NIN };
enum { GEOSRAD_SWD_C_CO2, GEOSRAD_SWD_C_O2, GEOSRAD_SWD_C_AIRMW, GEOSRAD_SWD_C_H2OMW, GEOSRAD_SWD_C_O3MW, GEOSRAD_SWD_C_RGAS,
       GEOSRAD_SWD_C_GRAV, GEOSRAD_SWD_C_UNDEF, GEOSRAD_SWD_NCONST };
enum { GEOSRAD_SWD_FSW /*(ncol,LM+1) model ordering*/, GEOSRAD_SWD_FSC, GEOSRAD_SWD_FSWU, GEOSRAD_SWD_FSCU, GEOSRAD_SWD_NIRR,
       GEOSRAD_SWD_NIRF, GEOSRAD_SWD_PARR, GEOSRAD_SWD_PARF, GEOSRAD_SWD_UVRR, GEOSRAD_SWD_UVRF, GEOSRAD_SWD_FSWBAND /*(ncol,14)*/,
       GEOSRAD_SWD_CLDTS, GEOSRAD_SWD_CLDHS, GEOSRAD_SWD_CLDMS, GEOSRAD_SWD_CLDLS, GEOSRAD_SWD_COTTP, GEOSRAD_SWD_COTHP,
       GEOSRAD_SWD_COTMP, GEOSRAD_SWD_COTLP,
       /* the no-aerosol flavour (FSWNAN ... of the GridComp, which calls the whole of SORADCORE a second time for them,
        * GEOS_SolarGridComp.F90:3249-3259): requested by a non-NULL pointer; validation, setcoef and McICA are shared with the
        * with-aerosol pass, only the band sweeps are repeated */
       GEOSRAD_SWD_FSWNA, GEOSRAD_SWD_FSCNA, GEOSRAD_SWD_FSWUNA, GEOSRAD_SWD_FSCUNA, GEOSRAD_SWD_FSWBANDNA /*(ncol,14)*/,
       GEOSRAD_SWD_NOUT };
int geosrad_sw_driver_rrtmg_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int nb_aer, const void *const *in,
                                const double *consts, int iceflgsw, int liqflgsw, double sc, double dist, int isolvar, int dyofyr,
                                int include_aerosols, int lcldlm, int lcldmh, int normflx, const void *bndsolvar,
                                const void *indsolvar, void *const *out);

/* geosrad_sw_driver_chou_dev: the Chou-Suarez branch of SORADCORE on the packed daytime columns (GEOS_SolarGridComp.F90:4484-4553
 * prep: interface pressures in hPa, odd oxygen -> non-negative ozone mass fraction, the species arrays QQ3 / RR3 with MAPL_UNDEF radii
 * replaced, zero aerosol arrays when there are none; :4558-4572 `call shrtwave` = SHRTWAVE :6597-6672 = `call SORAD`).  Fields in the
 * GEOS layout and MODEL ordering (what sorad expects).  The RADSW_BINARY_CLOUDS option (:4480-4481) is the caller's `where`.
 * taua / ssaa / asya (ncol,LM,8) in sorad's (tau, tau*ssa, tau*ssa*g) form, or all three NULL (num_aero_vars == 0).  hk_uv (5),
 * hk_ir (3,10): HOST pointers, the GridComp's HK_UV_TEMP / HK_IR_TEMP (:2997-3028).  lcldmh / lcldlm: sorad's ict / icb.
 * Outputs as SHRTWAVE's: FSW, FSC, FSWU, FSCU (ncol,LM+1), the six surface components (ncol), FSWBAND (ncol,8); DRBAND / DFBAND
 * (ncol,8) are written when do_drfband != 0 (SOLAR_TO_OBIO .and. include_aerosols), else may be NULL.  Fractions of the TOA insolation. */
enum { GEOSRAD_SWC_PLE /*(ncol,LM+1) Pa*/, GEOSRAD_SWC_T, GEOSRAD_SWC_Q, GEOSRAD_SWC_OX, GEOSRAD_SWC_CL, GEOSRAD_SWC_QI, GEOSRAD_SWC_QL,
       GEOSRAD_SWC_QR, GEOSRAD_SWC_QS, GEOSRAD_SWC_RI /*m, MAPL_UNDEF allowed*/, GEOSRAD_SWC_RL, GEOSRAD_SWC_RR, GEOSRAD_SWC_RS,
       GEOSRAD_SWC_TAUA /*(ncol,LM,8) nullable*/, GEOSRAD_SWC_SSAA, GEOSRAD_SWC_ASYA, GEOSRAD_SWC_ZT /*cos zenith*/, GEOSRAD_SWC_ALBVR,
       GEOSRAD_SWC_ALBVF, GEOSRAD_SWC_ALBNR, GEOSRAD_SWC_ALBNF, GEOSRAD_SWC_NIN };
enum { GEOSRAD_SWC_C_CO2, GEOSRAD_SWC_C_O3MW, GEOSRAD_SWC_C_AIRMW, GEOSRAD_SWC_C_UNDEF, GEOSRAD_SWC_NCONST };
enum { GEOSRAD_SWC_FSW, GEOSRAD_SWC_FSC, GEOSRAD_SWC_FSWU, GEOSRAD_SWC_FSCU, GEOSRAD_SWC_NIRR, GEOSRAD_SWC_NIRF, GEOSRAD_SWC_PARR,
       GEOSRAD_SWC_PARF, GEOSRAD_SWC_UVRR, GEOSRAD_SWC_UVRF, GEOSRAD_SWC_FSWBAND, GEOSRAD_SWC_DRBAND, GEOSRAD_SWC_DFBAND, GEOSRAD_SWC_NOUT };
int geosrad_sw_driver_chou_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, const void *const *in, const double *consts,
                               int lcldmh, int lcldlm, const void *hk_uv, const void *hk_ir, int do_drfband, void *const *out);

/* geosrad_sw_driver_chou_na_dev: geosrad_sw_driver_chou_dev + the aerosol-free internals FSWNAN, FSCNAN, FSWUNAN, FSCUNAN, FSWBANDNAN the
 * GridComp obtains from a second SORADCORE with include_aerosols = .false. (GEOS_SolarGridComp.F90:3249-3259, :3997-4016, :4541-4551),
 * from one k_swc_prep and one shared solver call (geosrad_sorad_na_dev).
 *   na_out: HOST array of GEOSRAD_SWCNA_NOUT device pointers: FSWNA, FSCNA, FSWUNA, FSCUNA (ncol,LM+1), FSWBANDNA (ncol,8), each bit for
 *   bit the FSW, FSC, FSWU, FSCU, FSWBAND of geosrad_sw_driver_chou_dev called with TAUA = SSAA = ASYA = NULL.  Any member may be NULL
 *   (left untouched); na_out NULL or all members NULL: the plain driver.
 * With the aerosol inputs NULL no second pass runs: the aerosol-free outputs are copies of their twins in `out`.  DRBAND / DFBAND keep their
 * do_drfband meaning and are never produced by the aerosol-free pass (:4010-4016).  `out` is bit for bit the plain driver's. */
enum { GEOSRAD_SWCNA_FSWNA, GEOSRAD_SWCNA_FSCNA, GEOSRAD_SWCNA_FSWUNA, GEOSRAD_SWCNA_FSCUNA, GEOSRAD_SWCNA_FSWBANDNA /*(ncol,8)*/,
       GEOSRAD_SWCNA_NOUT };
int geosrad_sw_driver_chou_na_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, const void *const *in, const double *consts,
                                  int lcldmh, int lcldlm, const void *hk_uv, const void *hk_ir, int do_drfband, void *const *out,
                                  void *const *na_out);

/* geosrad_lw_update_flx_dev: Update_Flx (GEOS_IrradGridComp.F90:3796-3999), the per-model-step linearisation of the LW fluxes in
 * the surface temperature.  rrtmg != 0: the no-aerosol flavours are `undef` and their internals may be NULL (IRR:3927-3990).
 * rrtmg = 0 reads FLXA_INT .. DFDTSCNA as real fields (the Chou-Suarez semantics): what an RRTMG caller passes who has filled them with
 * geosrad_lw_driver_rrtmg_na_dev, for FLXA, FLA, OLRA / OLA, LWSA / LAS, FLNSNA / FLNSA.
 * lev_mid_high / lev_low_mid: the model levels found from PREF (IRR:3811-3829). */
enum { GEOSRAD_LWU_TSINST, GEOSRAD_LWU_TS_INT, GEOSRAD_LWU_SFCEM_INT, GEOSRAD_LWU_FCLD, GEOSRAD_LWU_FLX_INT, GEOSRAD_LWU_FLXA_INT,
       GEOSRAD_LWU_FLC_INT, GEOSRAD_LWU_FLA_INT, GEOSRAD_LWU_FLXU_INT, GEOSRAD_LWU_FLXAU_INT, GEOSRAD_LWU_FLCU_INT,
       GEOSRAD_LWU_FLAU_INT, GEOSRAD_LWU_FLXD_INT, GEOSRAD_LWU_FLXAD_INT, GEOSRAD_LWU_FLCD_INT, GEOSRAD_LWU_FLAD_INT,
       GEOSRAD_LWU_DFDTS, GEOSRAD_LWU_DFDTSNA, GEOSRAD_LWU_DFDTSC, GEOSRAD_LWU_DFDTSCNA, GEOSRAD_LWU_NIN };
enum { GEOSRAD_LWU_FLX, GEOSRAD_LWU_FLXA, GEOSRAD_LWU_FLC, GEOSRAD_LWU_FLA, GEOSRAD_LWU_FLXU, GEOSRAD_LWU_FLXAU, GEOSRAD_LWU_FLCU,
       GEOSRAD_LWU_FLAU, GEOSRAD_LWU_FLXD, GEOSRAD_LWU_FLXAD, GEOSRAD_LWU_FLCD, GEOSRAD_LWU_FLAD, GEOSRAD_LWU_OLR, GEOSRAD_LWU_OLRA,
       GEOSRAD_LWU_OLC, GEOSRAD_LWU_OLA, GEOSRAD_LWU_OLCC5, GEOSRAD_LWU_DSFDTS, GEOSRAD_LWU_SFCEM, GEOSRAD_LWU_LWS, GEOSRAD_LWU_LWSA,
       GEOSRAD_LWU_LCS, GEOSRAD_LWU_LAS, GEOSRAD_LWU_LCSC5, GEOSRAD_LWU_FLNS, GEOSRAD_LWU_FLNSNA, GEOSRAD_LWU_FLNSC, GEOSRAD_LWU_FLNSA,
       GEOSRAD_LWU_DSFDTS0, GEOSRAD_LWU_SFCEM0, GEOSRAD_LWU_TSREFF, GEOSRAD_LWU_CLDTT, GEOSRAD_LWU_NOUT };
int geosrad_lw_update_flx_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int rrtmg, int lev_mid_high, int lev_low_mid,
                              double undef, const void *const *in, void *const *out);

/* geosrad_lw_update_rats_dev: the RATS exports of Update_Flx (GEOS_IrradGridComp.F90:4036-4120): for every listed gas n, from the
 * INTERNAL state with and without the gas: dOLR_n, dLWS_n, dFLNS_n, dSFCEM_n, NETTRAP_n (ncol,nrats); COLTRAP_n (ncol,LM,nrats);
 * FLX_n, DFDTS_n (ncol,0:LM,nrats).  Gas slowest, like the (IM,JM,0:LM,nRATS) internals; any output may be NULL. */
enum { GEOSRAD_LWR_FLX_INT /*(ncol,0:LM)*/, GEOSRAD_LWR_SFCEM_INT /*(ncol)*/, GEOSRAD_LWR_DFDTS, GEOSRAD_LWR_FLX_RAT /*(ncol,0:LM,nrats)*/,
       GEOSRAD_LWR_SFCEM_RAT /*(ncol,nrats)*/, GEOSRAD_LWR_DFDTS_RAT, GEOSRAD_LWR_NIN };
enum { GEOSRAD_LWR_DOLR, GEOSRAD_LWR_DLWS, GEOSRAD_LWR_DFLNS, GEOSRAD_LWR_DSFCEM, GEOSRAD_LWR_NETTRAP, GEOSRAD_LWR_COLTRAP, GEOSRAD_LWR_FLX,
       GEOSRAD_LWR_DFDTS_OUT, GEOSRAD_LWR_NOUT };
int geosrad_lw_update_rats_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int nrats, const void *const *in, void *const *out);

/* geosrad_lw_update_bands_dev: the band OLR / brightness-temperature exports of Update_Flx (GEOS_IrradGridComp.F90:3993-4021 with
 * Tbr_from_band_flux / invert_Planck_for_T, :4132-4208) for the bands selected by band_output[16]: OLRBbbRG = OLRB_int + DOLRB_int *
 * (TSINST - TS_INT); TBRBbbRG = narrow-band inversion of the Planck function in double precision, MAPL_UNDEF for a band whose updated
 * flux is zero everywhere (before the first full calculation).  olrb_int / dolrb_int: (16,ncol) as the driver returns them
 * (GEOSRAD_LWD_OLRB / _DOLRB); olrb_exp / tbrb_exp: (ncol,16), band bb's export is the contiguous slice bb, either may be NULL;
 * wavenum1 / wavenum2: rrlw_wvn's band limits in cm-1 (host). */
int geosrad_lw_update_bands_dev(geosrad_ctx *ctx, void *stream, int ncol, const int32_t *band_output, const double *wavenum1,
                                const double *wavenum2, double undef, const void *tsinst, const void *ts_int, const void *olrb_int,
                                const void *dolrb_int, void *olrb_exp, void *tbrb_exp);

/* geosrad_sw_update_export_dev: the flux part of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7540-7579): exports = normalised
 * internals x SLR (3-D net / up / down, per-band, TOA and surface). */
enum { GEOSRAD_SWU_SLR, GEOSRAD_SWU_FSWN, GEOSRAD_SWU_FSCN, GEOSRAD_SWU_FSWNAN, GEOSRAD_SWU_FSCNAN, GEOSRAD_SWU_FSWUN,
       GEOSRAD_SWU_FSCUN, GEOSRAD_SWU_FSWUNAN, GEOSRAD_SWU_FSCUNAN, GEOSRAD_SWU_FSWBANDN, GEOSRAD_SWU_FSWBANDNAN, GEOSRAD_SWU_NIN };
enum { GEOSRAD_SWU_FSW, GEOSRAD_SWU_FSC, GEOSRAD_SWU_FSWNA, GEOSRAD_SWU_FSCNA, GEOSRAD_SWU_FSWU, GEOSRAD_SWU_FSCU, GEOSRAD_SWU_FSWUNA,
       GEOSRAD_SWU_FSCUNA, GEOSRAD_SWU_FSWD, GEOSRAD_SWU_FSCD, GEOSRAD_SWU_FSWDNA, GEOSRAD_SWU_FSCDNA, GEOSRAD_SWU_FSWBAND,
       GEOSRAD_SWU_FSWBANDNA, GEOSRAD_SWU_RSR, GEOSRAD_SWU_RSC, GEOSRAD_SWU_RSRNA, GEOSRAD_SWU_RSCNA, GEOSRAD_SWU_RSRS, GEOSRAD_SWU_RSCS,
       GEOSRAD_SWU_RSRSNA, GEOSRAD_SWU_RSCSNA, GEOSRAD_SWU_OSR, GEOSRAD_SWU_OSRCLR, GEOSRAD_SWU_OSRNA, GEOSRAD_SWU_OSRCNA,
       GEOSRAD_SWU_NOUT };
int geosrad_sw_update_export_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int nbands, const void *const *in,
                                 void *const *out);

/* ---- the ocean-biology coupling (USE_OCEANOBIOGEOCHEM: 1 -> SOLAR_TO_OBIO) ---------------------------------------------------------
 * geosrad_obio_weights: the band bookkeeping of UPDATE_EXPORT's SOLAR TO OBIO conversion (GEOS_SolarGridComp.F90:7584-7737) on the host;
 * no device and no context are needed (ctx-less: geosrad_last_error(NULL) gives this thread's last complaint).  The solver's bands are
 * walked together with the 33 OBIO bands (OBIO_bands_nm, :6794-6835; OBIO_bands_wavenum = 1.e7 / OBIO_bands_nm(2:1:-1,:)) in increasing
 * wavenumber (:7665-7728, with its early exits, the kb_start carry and both continuity checks); every overlapping pair contributes
 * sfrac = (min(swvn2,owvn2) - max(swvn1,owvn1)) / (swvn2 - swvn1).  Every operation is made in real_kind (4 float, 8 double).
 *   scheme GEOSRAD_OBIO_RRTMG: rrsw_wvn's wavenum1/2(16:29), order 14, 1..13 (:7636-7648); nbands must be 14
 *          GEOSRAD_OBIO_CHOU : 1.e7 / CHOU_bands_nm (:6838-6847, band 2 = 285-300 nm), order 8..1 (:7652-7661); nbands must be 8
 *          GEOSRAD_OBIO_BANDS: the caller's limits wvn1 / wvn2 [cm-1] (nbands) and `order`, the 1-based band numbers in increasing
 *                              wavenumber (what the RRTMGP branch takes from its k-distribution, :7624-7628); 1 <= nbands <= 16
 *   For the two built-in schemes wvn1 / wvn2 / order are ignored and may be NULL.
 *   weights (33, nbands), OBIO band fastest: sfrac of the pair in real_kind widened to double, 0 where the bands do not overlap;
 *   npairs: the number of overlaps (46 for RRTMG, 39 for Chou-Suarez).  Either may be NULL.
 * GEOSRAD_EINVAL with the reference's text where it asserts ('SOLAR bands not complete and unique!', 'OBIO bands not complete and
 * unique!'), and for a bad scheme / real_kind / nbands, wvn1 >= wvn2, or an `order` that is no permutation of 1..nbands. */
enum { GEOSRAD_OBIO_CHOU, GEOSRAD_OBIO_RRTMG, GEOSRAD_OBIO_BANDS };
enum { GEOSRAD_NB_OBIO = 33, GEOSRAD_OBIO_MAXBANDS = 16 };
int geosrad_obio_weights(int scheme, int real_kind, int nbands, const double *wvn1, const double *wvn2, const int32_t *order,
                         double *weights /* (33, nbands), OBIO band fastest */, int32_t *npairs);

/* geosrad_sw_update_obio_dev: the conversion itself (GEOS_SolarGridComp.F90:7584-7737), every model step over all columns:
 * DROBIO(:,:,kb) = SLR * sum over the overlapping solar bands ib, in increasing wavenumber, of DRBANDN(:,:,ib) * sfrac, the accumulator
 * starting from zero (:7666-7667, :7719-7720, :7731-7734); DFOBIO likewise from DFBANDN.  Bit for bit the Fortran statements without
 * contraction.  scheme / nbands / wvn1 / wvn2 / order (host) as for geosrad_obio_weights.  slr (ncol), drbandn / dfbandn (ncol,nbands)
 * as the drivers return DRBAND / DFBAND, drobio / dfobio (ncol,33): device pointers of the context's real kind.  A NULL output is "not
 * associated" and skipped; with both NULL nothing is launched and the call returns GEOSRAD_OK.  No solver tables are needed; the call does
 * not synchronise.  GEOSRAD_EINVAL, nothing launched: slr or the matching input NULL while its output is requested, ncol < 1, or anything
 * geosrad_obio_weights rejects. */
int geosrad_sw_update_obio_dev(geosrad_ctx *ctx, void *stream, int ncol, int scheme, int nbands, const double *wvn1, const double *wvn2,
                               const int32_t *order, const void *slr, const void *drbandn, const void *dfbandn, void *drobio,
                               void *dfobio);

/* geosrad_sw_update_surface_dev: the 2-D block of UPDATE_EXPORT above the flux part (GEOS_SolarGridComp.F90:7403-7533): the four
 * albedo exports (import where SLR > 0, else MAPL_UNDEF), the total surface albedo ALB / ALBEDO (:7458-7465), the incident and
 * surface fluxes SLRTP, DR/DF UVR PAR NIR, the normal-incidence DRN*, SLRSF*, SLRSUF* (with SLN = SLR / ZTH where ZTH > 0, :6877-6881).
 * in: (ncol) fields, FSWN / FSCN / FSWNAN / FSCNAN (ncol,0:LM) (the last three only for the exports that read them). */
enum { GEOSRAD_SWS_SLR, GEOSRAD_SWS_ZTH, GEOSRAD_SWS_ALBVF, GEOSRAD_SWS_ALBVR, GEOSRAD_SWS_ALBNF, GEOSRAD_SWS_ALBNR, GEOSRAD_SWS_DRUVRN,
       GEOSRAD_SWS_DFUVRN, GEOSRAD_SWS_DRPARN, GEOSRAD_SWS_DFPARN, GEOSRAD_SWS_DRNIRN, GEOSRAD_SWS_DFNIRN, GEOSRAD_SWS_FSWN, GEOSRAD_SWS_FSCN,
       GEOSRAD_SWS_FSWNAN, GEOSRAD_SWS_FSCNAN, GEOSRAD_SWS_NIN };
enum { GEOSRAD_SWS_ALBVF_X, GEOSRAD_SWS_ALBVR_X, GEOSRAD_SWS_ALBNF_X, GEOSRAD_SWS_ALBNR_X, GEOSRAD_SWS_ALBEDO, GEOSRAD_SWS_SLRTP,
       GEOSRAD_SWS_DRUVR, GEOSRAD_SWS_DFUVR, GEOSRAD_SWS_DRPAR, GEOSRAD_SWS_DFPAR, GEOSRAD_SWS_DRNIR, GEOSRAD_SWS_DFNIR, GEOSRAD_SWS_DRNUVR,
       GEOSRAD_SWS_DRNPAR, GEOSRAD_SWS_DRNNIR, GEOSRAD_SWS_SLRSF, GEOSRAD_SWS_SLRSFC, GEOSRAD_SWS_SLRSFNA, GEOSRAD_SWS_SLRSFCNA,
       GEOSRAD_SWS_SLRSUF, GEOSRAD_SWS_SLRSUFC, GEOSRAD_SWS_SLRSUFNA, GEOSRAD_SWS_SLRSUFCNA, GEOSRAD_SWS_NOUT };
int geosrad_sw_update_surface_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, double undef, const void *const *in, void *const *out);

/* geosrad_sw_update_clouds_dev: the cloud diagnostics of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7006-7058, :7223-7392), every model step
 * over all columns: super-layer cloud fractions CLD?? / COTDEN?? (max of FCLD over layers 1..lcldmh-1, lcldmh..lcldlm-1, lcldlm..LM;
 * CLDTT = 1 - (1-HI)(1-MD)(1-LO)), GETVISTAU's diffuse optical thickness per species (called with ict = lcldmh, icb = lcldlm, :7264-7272;
 * dp in Pa, radii x 1e6 with no MAPL_UNDEF substitution), its super-layer sums TAU??, TAUTX, COT?? (MAPL_UNDEF where the fraction is 0),
 * COTNUM??, and the cloud top CLDTMP / CLDPRS: T and the upper interface pressure of the topmost layer whose total optical thickness
 * exceeds taucrit (the TAUCRIT: resource, default 0.10), MAPL_UNDEF where none does.  ZTH as MAPL_SunGetInsolation returns it (after
 * max(ZTH,0), :6874, it enters only GETVISTAU's beam scaling, which no export reads: it may be NULL).  Fields (ncol,LM), PLE (ncol,0:LM)
 * in Pa, the 2-D exports and ZTH (ncol); radii in m.  A NULL output is "not associated" and left untouched.  GEOSRAD_EINVAL, nothing
 * launched: an input a requested output needs is NULL (FCLD for all; PLE, QI..QS, RI..RS for all but FCLD_X / CLD?? / COTDEN??; T for
 * CLDTMP), ncol or lm < 1, not 1 < lcldmh < lcldlm <= lm (SOL:3036-3062), or the Chou-Suarez SW tables are not set. */
enum { GEOSRAD_SWK_FCLD /*(ncol,LM)*/, GEOSRAD_SWK_PLE /*(ncol,0:LM) Pa*/, GEOSRAD_SWK_T, GEOSRAD_SWK_QI, GEOSRAD_SWK_QL, GEOSRAD_SWK_QR,
       GEOSRAD_SWK_QS, GEOSRAD_SWK_RI /*m*/, GEOSRAD_SWK_RL, GEOSRAD_SWK_RR, GEOSRAD_SWK_RS, GEOSRAD_SWK_ZTH /*(ncol)*/, GEOSRAD_SWK_NIN };
enum { GEOSRAD_SWK_C_GRAV, GEOSRAD_SWK_C_UNDEF, GEOSRAD_SWK_NCONST };
enum { GEOSRAD_SWK_FCLD_X /*(ncol,LM)*/, GEOSRAD_SWK_TAUCLI, GEOSRAD_SWK_TAUCLW, GEOSRAD_SWK_TAUCLR, GEOSRAD_SWK_TAUCLS,
       GEOSRAD_SWK_CLDLO /*(ncol)*/, GEOSRAD_SWK_CLDMD, GEOSRAD_SWK_CLDHI, GEOSRAD_SWK_CLDTT, GEOSRAD_SWK_COTDENLO, GEOSRAD_SWK_COTDENMD,
       GEOSRAD_SWK_COTDENHI, GEOSRAD_SWK_COTDENTT, GEOSRAD_SWK_TAULO, GEOSRAD_SWK_TAUMD, GEOSRAD_SWK_TAUHI, GEOSRAD_SWK_TAUTT,
       GEOSRAD_SWK_TAUTX, GEOSRAD_SWK_COTLO, GEOSRAD_SWK_COTMD, GEOSRAD_SWK_COTHI, GEOSRAD_SWK_COTTT, GEOSRAD_SWK_COTNUMLO,
       GEOSRAD_SWK_COTNUMMD, GEOSRAD_SWK_COTNUMHI, GEOSRAD_SWK_COTNUMTT, GEOSRAD_SWK_CLDTMP, GEOSRAD_SWK_CLDPRS, GEOSRAD_SWK_NOUT };
int geosrad_sw_update_clouds_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int lcldmh, int lcldlm, double taucrit,
                                 const double *consts /*GRAV, UNDEF*/, const void *const *in, void *const *out);

/* geosrad_sw_update_cldhb_dev: the heartbeat McICA cloud fractions CLD??SWHB of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7060-7223, inside
 * #ifdef SOLAR_RADVAL), every model step over all columns.  For every column with any FCLD > 0: the generator inputs from the imports
 * (:7133-7161: plmid = 0.5 (PLE(k-1) + PLE(k)), play = plmid / 100, cfac = 1.02 * 100 * (PLE(k) - PLE(k-1)), ciwp / clwp = cfac QI / QL,
 * interior interface temperatures weighted by cfac, zmid from the hydrostatic equation with zmid(LM) = 0), generate_stochastic_clouds
 * with the 112 g-points of RRTMG_SW as sub-columns, cwp_tiny = 1e-20 and seed_order = [4,3,2,1] in the MODEL's vertical ordering (TOA at
 * layer 1: the levels are not reversed, :7125-7131), clearCounts_threeBand(cloudLM = lcldlm, cloudMH = lcldmh) (high = layers
 * 1..lcldmh-1, middle = lcldmh..lcldlm-1, low = lcldlm..LM) and CLD?? = 1 - count / 112 (:7187-7206); columns without cloud fraction
 * get 0 (:7077-7080).  No sub-column array is materialised.  The context's condensate inhomogeneity (geosrad_set_inhomogeneity) and
 * correlation lengths (geosrad_set_corr_lengths) apply, as in geosrad_mcica_dev; no solver tables are needed.  Fields (ncol,LM), PLE
 * (ncol,0:LM) in Pa, LATS (ncol) in radians, the exports (ncol).  consts NULL: MAPL_GRAV = 9.80665, MAPL_RGAS = 8314.47 / 28.965.
 * A NULL output is "not associated" and left untouched; with all four NULL nothing is launched and the call returns GEOSRAD_OK.
 * GEOSRAD_EINVAL, nothing launched: an input is NULL while an output is requested, ncol < 1, lm < 4 (the seeds need four layers), or
 * not 1 < lcldmh < lcldlm <= lm (SOL:3036-3062). */
enum { GEOSRAD_SWHB_FCLD /*(ncol,LM)*/, GEOSRAD_SWHB_PLE /*(ncol,0:LM) Pa*/, GEOSRAD_SWHB_T, GEOSRAD_SWHB_QI, GEOSRAD_SWHB_QL,
       GEOSRAD_SWHB_LATS /*(ncol) radians*/, GEOSRAD_SWHB_NIN };
enum { GEOSRAD_SWHB_C_GRAV, GEOSRAD_SWHB_C_RGAS, GEOSRAD_SWHB_NCONST };
enum { GEOSRAD_SWHB_CLDTT /*(ncol)*/, GEOSRAD_SWHB_CLDHI, GEOSRAD_SWHB_CLDMD, GEOSRAD_SWHB_CLDLO, GEOSRAD_SWHB_NOUT };
int geosrad_sw_update_cldhb_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int lcldmh, int lcldlm, int doy,
                                const double *consts /*GRAV, RGAS; NULL: MAPL's values*/, const void *const *in, void *const *out);

/* geosrad_rad_tendencies_dev: the parent's heating rates (GEOS_RadiationGridComp.F90:798-819). */
enum { GEOSRAD_RT_PLE, GEOSRAD_RT_FLW, GEOSRAD_RT_FSW, GEOSRAD_RT_FLWCLR, GEOSRAD_RT_FSWCLR, GEOSRAD_RT_FSWNA, GEOSRAD_RT_FLA,
       GEOSRAD_RT_FSCNA, GEOSRAD_RT_DSFDTS, GEOSRAD_RT_SFCEM, GEOSRAD_RT_TRD, GEOSRAD_RT_NIN };
enum { GEOSRAD_RT_DTDT, GEOSRAD_RT_RADLW, GEOSRAD_RT_RADSW, GEOSRAD_RT_RADLWC, GEOSRAD_RT_RADSWC, GEOSRAD_RT_RADSWNA,
       GEOSRAD_RT_RADLWCNA, GEOSRAD_RT_RADSWCNA, GEOSRAD_RT_BLW, GEOSRAD_RT_ALW, GEOSRAD_RT_RADSRF, GEOSRAD_RT_NOUT };
int geosrad_rad_tendencies_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, double grav, double cp, const void *const *in,
                               void *const *out);

/* ---- lit-column compaction of the solar component ----------------------------------------------------------------------
 * GEOS_SolarGridComp.F90:3686 (`daytime = ZTH > 0.`, NumLit = count(daytime)) and PackIt / UnPackIt (:7753-7799): SORADCORE works on
 * the daytime columns only, packed to the front of every field in (i, j) order; on a node each GPU therefore takes its share of the
 * LIT columns.  All pointers are device pointers of the context's real kind (int32 for the index arrays).
 *   geosrad_lit_index_dev : lit_index[m] = column of packed position m (stable order), lit_pos[column] = packed position or -1,
 *                           *nlit_dev = NumLit; when nlit_host is not NULL the stream is synchronised and NumLit returned in it
 *   geosrad_lit_pack_dev  : Packed(m, l) = UnPacked(lit_index[m], l), l = 1..nlev; Packed is (pdim, nlev), UnPacked (udim, nlev)
 *   geosrad_lit_unpack_dev: UnPacked(lit_index[m], l) = Packed(m, l); dark columns receive `dflt` when use_default != 0
 *                           (UnPackIt's optional DEFAULT), otherwise they keep their values */
int geosrad_lit_index_dev(geosrad_ctx *ctx, void *stream, int ncol, const void *zth, int32_t *lit_index, int32_t *lit_pos,
                          int32_t *nlit_dev, int *nlit_host);
int geosrad_lit_pack_dev(geosrad_ctx *ctx, void *stream, int pdim, int udim, int nlev, const int32_t *lit_index, const int32_t *nlit_dev,
                         const void *unpacked, void *packed);
int geosrad_lit_unpack_dev(geosrad_ctx *ctx, void *stream, int pdim, int udim, int nlev, const int32_t *lit_pos, const void *packed,
                           void *unpacked, int use_default, double dflt);

/* ---- the SW branch of SORADCORE on the un-packed tile ------------------------------------------------------------------
 * geosrad_sw_driver_rrtmg_lit_dev / geosrad_sw_driver_chou_lit_dev: geosrad_sw_driver_rrtmg_dev / geosrad_sw_driver_chou_dev with
 * SORADCORE's PackIt of every import (GEOS_SolarGridComp.F90:3839-3894) and UnPackIt(..., DEFAULT) of every result (:6520-6580,
 * :7753-7799) inside: `in` and `out` (the same GEOSRAD_SWD_* / GEOSRAD_SWC_* orders) are fields of the whole tile, leading dimension
 * ncol = IM*JM; lit_index / lit_pos / nlit are what geosrad_lit_index_dev returned for `daytime = ZTH > 0.` (:3686) and are trusted; the
 * call does not synchronise.  The prep kernels read every import at column lit_index[m]; the solver runs on nlit columns with the
 * workspace contents of the packed route, so on a lit column every output is bit for bit what geosrad_lit_pack_dev of every input, the
 * packed driver and geosrad_lit_unpack_dev of every output give.  On a dark column output k receives dark[k] (host array in the output
 * enum's order, converted to the real kind: UnPackIt's DEFAULT, the internal spec's default, :6534) unless bit k of keep_mask is set, in
 * which case it keeps its value (an InOut internal, :6523-6524).  A NULL output stays "not associated".  With include_aerosols == 0 the
 * RRTMG driver leaves CLD?S of the lit columns alone, as the packed driver does (:6405).
 * The aerosol imports TAUA / SSAA / ASYA are READ ONLY here: the reference normalises its packed buffer (:6116-6125 act on BufInp), never
 * the import, whereas geosrad_sw_driver_rrtmg_dev, which is handed that buffer, normalises it in place.
 * The workspace is sized by nlit.  geosrad_set_chunk, the inhomogeneity and correlation-length settings, GEOSRAD_SW_PATH and
 * geosrad_set_overcast apply as for the packed drivers.  nlit == 0: no solver kernel runs, the dark values are written, GEOSRAD_OK.
 * GEOSRAD_EINVAL (GEOSRAD_EINPUT where the packed driver gives that), nothing launched: nlit < 0 or > ncol; lit_index or lit_pos NULL
 * with nlit > 0; lit_pos or dark NULL while a requested output has its keep bit clear; whatever the packed driver or its solver rejects
 * (isolvar == 1 for RRTMG).  The Chou-Suarez driver wants all of FSW .. FSWBAND (and DRBAND / DFBAND with do_drfband), like sorad; with
 * do_drfband == 0 it neither writes nor fills DRBAND / DFBAND and asks nothing of their dark values. */
int geosrad_sw_driver_rrtmg_lit_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos,
                                    int lm, int nb_aer, const void *const *in, const double *consts, int iceflgsw, int liqflgsw, double sc,
                                    double dist, int isolvar, int dyofyr, int include_aerosols, int lcldlm, int lcldmh, int normflx,
                                    const void *bndsolvar, const void *indsolvar, const double *dark /*[GEOSRAD_SWD_NOUT]*/,
                                    uint64_t keep_mask, void *const *out);
int geosrad_sw_driver_chou_lit_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos,
                                   int lm, const void *const *in, const double *consts, int lcldmh, int lcldlm, const void *hk_uv,
                                   const void *hk_ir, int do_drfband, const double *dark /*[GEOSRAD_SWC_NOUT]*/, uint64_t keep_mask,
                                   void *const *out);

/* geosrad_sw_driver_chou_na_lit_dev: geosrad_sw_driver_chou_lit_dev + the aerosol-free internals of geosrad_sw_driver_chou_na_dev on the
 * un-packed tile.  na_out (GEOSRAD_SWCNA_* order) are fields of the whole tile like `out`; on a lit column each is bit for bit what the
 * pack / geosrad_sw_driver_chou_na_dev / unpack route gives, and they ride the same un-packing kernel as `out`.  On a dark column
 * na_out[k] receives dark_na[k] (host array [GEOSRAD_SWCNA_NOUT]: UnPackIt's DEFAULT of FSWNAN ..., :6534) unless bit k of keep_na is
 * set.  nlit == 0: the dark values of `out` and na_out are written and nothing else runs.  GEOSRAD_EINVAL, nothing launched: what
 * geosrad_sw_driver_chou_lit_dev rejects; lit_pos or dark_na NULL while a requested (non-NULL) member of na_out has its keep bit clear. */
int geosrad_sw_driver_chou_na_lit_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos,
                                      int lm, const void *const *in, const double *consts, int lcldmh, int lcldlm, const void *hk_uv,
                                      const void *hk_ir, int do_drfband, const double *dark /*[GEOSRAD_SWC_NOUT]*/, uint64_t keep_mask,
                                      void *const *out, const double *dark_na /*[GEOSRAD_SWCNA_NOUT]*/, int keep_na, void *const *na_out);

/* geosrad_sw_driver_rrtmg_obio_dev / geosrad_sw_driver_rrtmg_obio_lit_dev: geosrad_sw_driver_rrtmg_dev / geosrad_sw_driver_rrtmg_lit_dev
 * with the per-band surface beam and diffuse fluxes a coupled ocean biology needs, the internals DRBANDN / DFBANDN
 * (GEOS_SolarGridComp.F90:778-796, :4148-4151): drband / dfband (ncol,14), fractions of the TOA insolation like FSWBAND, both given or both
 * NULL (else GEOSRAD_EINVAL; both NULL = the plain driver).  When they are given and include_aerosols != 0 the with-aerosol rrtmg_sw call
 * runs with do_drfband = SOLAR_TO_OBIO .and. include_aerosols (:6385) and writes them; with include_aerosols == 0 the two arrays are left
 * untouched on lit and dark columns alike (the reference does not compute them in its no-aerosol call, :4010-4016).  The no-aerosol second
 * pass never computes them.  Every output of `out` is bit for bit what the plain entry point returns.  On the tile: dark_obio[2] (host) are
 * UnPackIt's DEFAULTs of DRBAND, DFBAND; bits 0, 1 of keep_obio make their dark columns keep their values; dark_obio may be NULL when both
 * bits are set. */
int geosrad_sw_driver_rrtmg_obio_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, int nb_aer, const void *const *in,
                                     const double *consts, int iceflgsw, int liqflgsw, double sc, double dist, int isolvar, int dyofyr,
                                     int include_aerosols, int lcldlm, int lcldmh, int normflx, const void *bndsolvar,
                                     const void *indsolvar, void *const *out, void *drband, void *dfband);
int geosrad_sw_driver_rrtmg_obio_lit_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlit, const int32_t *lit_index, const int32_t *lit_pos,
                                         int lm, int nb_aer, const void *const *in, const double *consts, int iceflgsw, int liqflgsw,
                                         double sc, double dist, int isolvar, int dyofyr, int include_aerosols, int lcldlm, int lcldmh,
                                         int normflx, const void *bndsolvar, const void *indsolvar, const double *dark /*[GEOSRAD_SWD_NOUT]*/,
                                         uint64_t keep_mask, void *const *out, const double *dark_obio /*[2]*/,
                                         int keep_obio /*bit 0 DRBAND, bit 1 DFBAND*/, void *drband, void *dfband);

#ifdef __cplusplus
}
#endif
#endif /* GEOSRAD_H */
