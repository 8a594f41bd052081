/* geosrad_radar.h -- C ABI of the front end of the radar simulator (CloudSat) of GEOSsatsim_GridComp's COSP, as entry points of libgeosrad.so.
 * The sixth public header beside geosrad.h, geosrad_gettau.h, geosrad_satsim.h, geosrad_misr_modis.h and geosrad_lidar.h: same library, same
 * geosrad_ctx, same conventions (real_kind fixes the element type of every `const void *` / `void *` real array; arrays in the reference's
 * Fortran layouts, the point index the fastest; level 1 is the top of the atmosphere; any output may be NULL = not wanted; 0 or a GEOSRAD_E*
 * code, the text from geosrad_last_error).
 *
 *   geosrad_prec_scops[_dev]     <- prec_scops, llnl/prec_scops.f:25-267
 *   geosrad_cosp_sghydro[_dev]   <- the sub-grid hydrometeor contents of cosp_iter, cosp.F90:399-519, with use_precipitation_fluxes = .false.
 *                                   (GEOS_SatsimGridComp.F90:3470)
 *   geosrad_radar_gases[_dev]    <- gases, quickbeam/gases.f90, for every volume, and path_integral with avint, quickbeam/math_lib.f90:96-155,
 *                                   :160-393, for every gate, as radar_simulator.f90:470-484 calls them on the matrices cosp_radar.F90:136-144
 *                                   makes
 *
 * This is the half of the radar whose results do not depend on the order of the points.  Not built: the reflectivity itself - dsd, zeff and
 * the Mie sum with the hp%Ze_scaled cache (radar_simulator.f90:258, :434-457), the CFAD and cosp_lidar_only_cloud statistics with CLCALIPSO2
 * and CLTLIDARRADAR - and the flux mode (pf_to_mr, cosp_precip_mxratio, cosp.F90:521-555), which GEOS does not use.  None of it needs a file:
 * GEOS sets use_mie_tables = 0 (GEOS_SatsimGridComp.F90:3545), and the nine hydrometeor classes are the HCLASS_* data statements of
 * cosp_constants.F90:108-127, which cosp_types.F90:1112-1126 hands to load_hydrometeor_classes.
 * The hydrometeor classes are counted in cosp_constants' I_* order (cosp_constants.F90:39-47). */
#ifndef GEOSRAD_RADAR_H
#define GEOSRAD_RADAR_H

#include "geosrad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mr_sub (npoints,nlev,9) and mr_hydro_sg (npoints,ncol,nlev,9): the I_* of cosp_constants.F90:39-47, from 0 */
enum { GEOSRAD_HYDRO_LSLIQ, GEOSRAD_HYDRO_LSICE, GEOSRAD_HYDRO_LSRAIN, GEOSRAD_HYDRO_LSSNOW, GEOSRAD_HYDRO_CVLIQ, GEOSRAD_HYDRO_CVICE,
       GEOSRAD_HYDRO_CVRAIN, GEOSRAD_HYDRO_CVSNOW, GEOSRAD_HYDRO_LSGRPL, GEOSRAD_NHYDRO };

/* geosrad_prec_scops[_dev]: prec_scops(npoints,nlev,ncol,ls_p_rate,cv_p_rate,frac_out,prec_frac), prec_scops.f:25-267, in its own argument
 * order.  ls_p_rate, cv_p_rate (npoints,nlev): only their sign is looked at (`.gt. 0.`).  frac_out (npoints,ncol,nlev): the SCOPS mask of
 * geosrad_scops[_dev], 0 clear, 1 stratiform, 2 convective; prec_frac (npoints,ncol,nlev): 0 clear, 1 large-scale, 2 convective, 3 both.  The
 * `_dev` variant holds both as one byte per cell, the host variant in the real kind, which is what a Fortran caller holds.
 * A level's large-scale precipitation goes, in this order, to the sub-columns with stratiform cloud in the level or large-scale
 * precipitation in the level above (possibilities ONE and TWO, :184-191); if there is none, to those with stratiform cloud in the level
 * below (THREE, :192-199; not asked at the last level, and the first level, :93-107, always has a level below: nlev >= 2); if none, to those
 * with stratiform cloud anywhere (Four, :200-207); if none, to all (Five, :208-213).  Convective precipitation the same on the convective
 * cloud (:216-262), its Five on the first cv_col sub-columns only: cv_col = 0.05*ncol, a product in the real kind truncated to an integer,
 * at least 1 (:54-55).
 * Errors: npoints < 1, nlev < 2, ncol outside 1..65535, a null array: GEOSRAD_EINVAL.
 * The `_dev` variant takes device pointers and is asynchronous on `stream`; its workspace (one byte per (point, sub-column)) is taken at the
 * first call and counted by geosrad_workspace_bytes.  The host variant stages the arrays through the chunked pipeline of the solver entry
 * points (geosrad_set_chunk applies; chunks and the shards of a geosrad_create_multi context split the points only) and returns the `_dev`
 * bits. */
int geosrad_prec_scops(geosrad_ctx *ctx, int npoints, int nlev, int ncol, const void *ls_p_rate, const void *cv_p_rate, const void *frac_out,
                       void *prec_frac);
int geosrad_prec_scops_dev(geosrad_ctx *ctx, void *stream, int npoints, int nlev, int ncol, const void *ls_p_rate, const void *cv_p_rate,
                           const void *frac_out_u8, void *prec_frac_u8);

/* geosrad_cosp_sghydro[_dev]: cosp.F90:399-519 on the SCOPS mask frac_out and the nine gridbox mixing ratios mr_* (npoints,nlev), kg/kg.
 * The four convective ones and mr_lsgrpl may be NULL = zero (GEOS zeroes the convective ones, GEOS_SatsimGridComp.F90:3687-3690).
 * Outputs: prec_frac (npoints,ncol,nlev): prec_scops on ls_p_rate = mr_lsrain + mr_lssnow + mr_lsgrpl and cv_p_rate = mr_cvrain + mr_cvsnow,
 * summed in the real kind in that order (:404-411); frac_ls, frac_cv, prec_ls, prec_cv (npoints,nlev): the number of sub-columns with
 * frac_out 1, frac_out 2, prec_frac 1 or 3, prec_frac 2 or 3, over ncol, in the real kind (:414-431); mr_sub (npoints,nlev,9): what every
 * sub-column of the matching kind carries - the gridbox value divided by its fraction where that fraction is not 0, by frac_ls / frac_cv
 * for the cloud classes, by prec_ls / prec_cv for the precipitation classes (:484-516; IEEE divisions in the real kind); and on request
 * mr_hydro_sg (npoints,ncol,nlev,9), the expanded array a Fortran caller knows as sghydro%mr_hydro: a stratiform cell carries the five ls
 * classes of mr_sub, a convective cell the four cv classes, every other entry is zero (:453-480).  At 97 200 x 30 x 72 that array is 7.5 GB:
 * it is written only when asked for, and nothing else reads it.
 * Oddities kept: the precipitation classes are assigned by the *cloud* mask frac_out, not by prec_frac (:473-480), and are then divided by
 * the fraction counted from prec_frac (:507-515).  So rain that falls below cloud base, in a clear cell, is in no sub-column - it is
 * dropped - and rain in a cloudy cell is scaled by the precipitating fraction, not the cloudy one.
 * Reff needs no output: a sub-column's radius is the gridbox one wherever its cell's kind matches, for the cloud and the precipitation
 * classes alike (:457-469), and nothing divides it.
 * Errors and staging as for geosrad_prec_scops[_dev]; a null mr_lsliq, mr_lsice, mr_lsrain or mr_lssnow is GEOSRAD_EINVAL.  The `_dev`
 * workspace adds one byte per cell (prec_frac, when it is not wanted as an output). */
int geosrad_cosp_sghydro(geosrad_ctx *ctx, int npoints, int nlev, int ncol, const void *frac_out, const void *mr_lsliq, const void *mr_lsice,
                         const void *mr_lsrain, const void *mr_lssnow, const void *mr_cvliq, const void *mr_cvice, const void *mr_cvrain,
                         const void *mr_cvsnow, const void *mr_lsgrpl, void *prec_frac, void *frac_ls, void *frac_cv, void *prec_ls,
                         void *prec_cv, void *mr_sub, void *mr_hydro_sg);
int geosrad_cosp_sghydro_dev(geosrad_ctx *ctx, void *stream, int npoints, int nlev, int ncol, const void *frac_out_u8, const void *mr_lsliq,
                             const void *mr_lsice, const void *mr_lsrain, const void *mr_lssnow, const void *mr_cvliq, const void *mr_cvice,
                             const void *mr_cvrain, const void *mr_cvsnow, const void *mr_lsgrpl, void *prec_frac_u8, void *frac_ls,
                             void *frac_cv, void *prec_ls, void *prec_cv, void *mr_sub, void *mr_hydro_sg);

/* geosrad_radar_gases[_dev]: the two-way gaseous attenuation of every volume and from the radar to every gate.  p (Pa), t (K), rh (%), zlev
 * (m), each (npoints,nlev) in the real kind; freq in GHz (Liebe's model holds below 300 GHz; CloudSat: 94); surface_radar 0 = spaceborne, the
 * gates counted from the top, 1 = at the surface, the gates counted from the surface (order_data, quickbeam/format_input.f90:66-130).
 * GEOS_SatsimGridComp never assigns surface_radar (declared :2858, passed :3613): what it runs with is whatever the compiler left there.
 * Outputs, `double` whatever the context's kind, because quickbeam is real*8 throughout: g_vol (npoints,nlev): gases() of the cell, dB/km
 * two-way (radar_simulator.f90:478-479); g_to_vol (npoints,nlev): path_integral(g_vol,hgt,1,k-1) for the cell's gate k (:480), in dB.
 * Arithmetic kept: the unit conversions p/100, zlev/1000, t - 273.15 are done in the real kind before widening (cosp_radar.F90:136-139) and
 * the + 273.15 in double (radar_simulator.f90:478); every literal of gases.f90 and its line tables are default-real constants widened, and
 * that is what is computed here.  path_integral's two branches: a path of at most 3 points is the sum of f(j) |s(2) - s(1)| - the first
 * spacing for every term; a longer one is AVINT on the sorted abscissas from the first to the last, whose brackets (ilo = 2, ihi = ntab - 2)
 * leave the two end intervals to the parabola next to them.  Its first gate is empty: g_to_vol is 0 there.  AVINT is evaluated directly for
 * every (point, gate) in the reference's order of operations, from parabola coefficients formed once a gate.
 * Height order: order_data takes every profile's order from the first profile; here zlev must decrease strictly with the level index at
 * every point, and still do so after the division by 1000 in the real kind - which is where AVINT would stop.
 * Errors: npoints < 1, nlev < 2, a surface_radar other than 0 or 1, freq <= 0, a null input: GEOSRAD_EINVAL.  A p or t <= 0 or heights that
 * do not decrease strictly set a flag on the device: the `_dev` variant reports it as GEOSRAD_EINPUT from geosrad_check with the array's
 * name (p, t, zlev), the host variant returns it.  The `_dev` workspace is five (npoints,nlev) planes of doubles; staging as above. */
int geosrad_radar_gases(geosrad_ctx *ctx, int npoints, int nlev, const void *p, const void *t, const void *rh, const void *zlev, double freq,
                        int surface_radar, void *g_vol, void *g_to_vol);
int geosrad_radar_gases_dev(geosrad_ctx *ctx, void *stream, int npoints, int nlev, const void *p, const void *t, const void *rh,
                            const void *zlev, double freq, int surface_radar, void *g_vol, void *g_to_vol);

#ifdef __cplusplus
}
#endif
#endif /* GEOSRAD_RADAR_H */
