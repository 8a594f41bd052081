/* geosrad_lidar.h -- C ABI of the lidar simulator (CALIPSO, PARASOL) of GEOSsatsim_GridComp's COSP, as entry points of libgeosrad.so.
 * The fifth public header beside geosrad.h, geosrad_gettau.h, geosrad_satsim.h and geosrad_misr_modis.h: same library, same geosrad_ctx,
 * same conventions (real_kind fixes the element type of every `const void *` / `void *` real array; arrays in the reference's Fortran
 * layouts, the point index the fastest; level 1 is the top of the atmosphere; any output may be NULL = not wanted; 0 or a GEOSRAD_E* code,
 * the text from geosrad_last_error).
 *
 *   geosrad_lidar[_dev]       <- COSP_LIDAR, cosp_lidar.F90:44-82, with lidar_simulator and parasol, actsim/lidar_simulator.F90:25-415,
 *                                :419-553, and diag_lidar, actsim/lmd_ipsl_stats.F90:34-179, as cosp_stats.F90:126-130 calls it when no
 *                                other vertical grid is used and :137-140 leaves its results
 *   geosrad_cosp_lidar_dev    <- call COSP with the ISCCP, MISR, MODIS and lidar simulators on: GEOS_SatsimGridComp.F90:3480-3516, :3722,
 *                                cosp_simulator.F90:113-126
 *
 * The reference counts its levels from the surface; here level 1 is the top, so its level k is level nlev+1-k and its presf(:,k) is
 * presf(:,nlev+2-k) of this header.  Its statements are reproduced operation by operation in the real kind: the layer thickness as the
 * difference of two heights summed from the surface up, the optical depths as running sums from the top, one for the molecules and one
 * for each of the four particle kinds.
 * Undefined is LIDAR_UNDEF = 999.999 inside and R_UNDEF = -1.0E30 in lidarcld, cldlayer, cfad_sr and parasolrefl, as cosp_stats.F90:137-140
 * leaves them.  Cloud fractions are fractions, not percent (the scaling of cosp_simulator.F90:160-165 hangs on flags GEOS_SatsimGridComp
 * never sets).  Not built: CLCALIPSO2 and CLTLIDARRADAR, which need the radar's reflectivity (geosrad_radar.h), and statistics on another grid
 * (cosp_change_vertical_grid; GEOS passes use_vgrid = .false., GEOS_SatsimGridComp.F90:3657). */
#ifndef GEOSRAD_LIDAR_H
#define GEOSRAD_LIDAR_H

#include "geosrad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cldlayer (npoints,4): the categories of COSP_CLDFRAC, lmd_ipsl_stats.F90:388-394, in its order */
enum { GEOSRAD_LIDAR_LOW, GEOSRAD_LIDAR_MID, GEOSRAD_LIDAR_HIGH, GEOSRAD_LIDAR_TOTAL, GEOSRAD_LIDAR_NCAT };

/* geosrad_lidar[_dev]: COSP_LIDAR (cosp_lidar.F90:44-82) and diag_lidar (lmd_ipsl_stats.F90:34-179) on gridbox-level fields and the SCOPS mask.
 * ice_type 0 = ice spheres, 1 = non-spherical ice (lidar_simulator.F90:206-241).  p (Pa, mid-layer), t (K), pplay (Pa, the pressure
 * COSP_CLDFRAC sorts the levels into low / mid / high by, :388-394; COSP passes gbx%ph, cosp_stats.F90:127), the water contents mr_* (kg/kg)
 * and the radii reff_* (metres) (npoints,nlev); presf (npoints,nlev+1) Pa, the layer edges from the top: presf(:,1) is what
 * cosp_lidar.F90:61 sets to 0, presf(:,2:nlev+1) what :60 takes from gbx%ph.  The thickness of layer k is
 * -(presf(k) - presf(k+1)) / (rhoair(k) 9.81) (lidar_simulator.F90:262-266).  land (npoints): 0 ocean, 1 land.  frac_out (npoints,ncol,nlev):
 * the SCOPS mask of geosrad_scops[_dev], 0 clear, 1 stratiform, 2 convective; the `_dev` variant holds it as one byte per cell, the host
 * variant in the real kind, which is what a Fortran caller holds.  The four convective arrays may be NULL = zero.
 * A sub-column's contents are formed by index from the mask, without the reference's (npoints,ncol,nlev,nhydro) array: a cell's stratiform /
 * convective fraction is the count of 1s / 2s in the mask over ncol; a stratiform cell carries mr_lsliq / frac_ls and mr_lsice / frac_ls,
 * a convective one mr_cvliq / frac_cv and mr_cvice / frac_cv, a clear one zeros (cosp.F90:414-431, :453-470, :484-494).  The radii are the
 * gridbox ones: COSP_LIDAR passes gbx%Reff (cosp_lidar.F90:73).  lidar_simulator accepts frac_out and never reads it (frac_sub,
 * lidar_simulator.F90:270), so the mask enters through the contents only.
 * Outputs: lidarcld (npoints,nlev), the fraction of the usable sub-columns (scattering ratio > 0.01) that are cloudy (> 5), R_UNDEF where
 * none is usable (lmd_ipsl_stats.F90:411-415); cldlayer (npoints,4), low, mid, high, total (:419-434); cfad_sr (npoints,15,nlev), the
 * fraction of the sub-columns in each scattering-ratio bin, upper edges 0.01, 1.2, 3, 5, 7, 10, 15, 20, 25, 30, 40, 50, 60, 80, 998.999
 * (:223-236; a larger ratio is in no bin), R_UNDEF on a level whose pmol is not positive; parasolrefl (npoints,5), the mean over the
 * sub-columns, summed in their order, of the PARASOL reflectance at solar zenith angles 0, 20, 40, 60, 80 degrees, R_UNDEF on land
 * (:162-176); pmol (npoints,nlev), the molecular attenuated backscatter.  Optional per sub-column: beta_tot (pnorm) and tau_tot
 * (npoints,ncol,nlev), refl (npoints,ncol,5).
 * A pnorm at or above 998.999 cannot occur for finite inputs, so a sub-column is undefined only where pmol disqualifies its level; what
 * lmd_ipsl_stats.F90:249-254 would add to a single undefined sub-column's cfad cell is not reproduced.
 * Errors: npoints < 1, nlev < 2, ncol outside 1..65535, an ice_type other than 0 or 1 (the reference then reads coefficients it never
 * set), a null input: GEOSRAD_EINVAL.  A pressure p or temperature t <= 0, or a pnorm that is not finite, sets a flag on the device:
 * the `_dev` variant reports it as GEOSRAD_EINPUT from geosrad_check with the array's name, the host variant returns it.
 * The `_dev` variant takes device pointers and is asynchronous on `stream`; its workspace (eleven (npoints,nlev) and two (npoints,ncol)
 * planes, one byte per cell and one per sub-column) is taken at the first call and counted by geosrad_workspace_bytes.  The host variant
 * stages the arrays through the chunked pipeline of the solver entry points (geosrad_set_chunk applies; chunks and the shards of a
 * geosrad_create_multi context split the points only) and returns the `_dev` bits. */
int geosrad_lidar(geosrad_ctx *ctx, int npoints, int nlev, int ncol, int ice_type, const void *p, const void *t, const void *presf,
                  const void *pplay, const void *frac_out, const void *mr_lsliq, const void *mr_lsice, const void *mr_cvliq,
                  const void *mr_cvice, const void *reff_lsliq, const void *reff_lsice, const void *reff_cvliq, const void *reff_cvice,
                  const void *land, void *lidarcld, void *cldlayer, void *cfad_sr, void *parasolrefl, void *pmol, void *beta_tot,
                  void *tau_tot, void *refl);
int geosrad_lidar_dev(geosrad_ctx *ctx, void *stream, int npoints, int nlev, int ncol, int ice_type, const void *p, const void *t,
                      const void *presf, const void *pplay, const void *frac_out_u8, const void *mr_lsliq, const void *mr_lsice,
                      const void *mr_cvliq, const void *mr_cvice, const void *reff_lsliq, const void *reff_lsice, const void *reff_cvliq,
                      const void *reff_cvice, const void *land, void *lidarcld, void *cldlayer, void *cfad_sr, void *parasolrefl,
                      void *pmol, void *beta_tot, void *tau_tot, void *refl);

/* geosrad_cosp_lidar_dev: call COSP with all four simulators on (USE_SATSIM = 1 also sets cfg%Llidar_sim, cfg%LCFADLIDARSR532 and
 * cfg%Lstats, GEOS_SatsimGridComp.F90:3498-3516), on GEOS fields in HBM, model order, nothing copied or flipped.  The arguments up to
 * modis_hist are those of geosrad_cosp_dev (geosrad_misr_modis.h), unchanged and in the same order; that entry point's own code runs, so
 * every ISCCP, MISR and MODIS output, the seeds and sgfcld are bit for bit its.  Then frocean (npoints) and ice_type (GEOS sets 0, :3535),
 * and the lidar's outputs in model order: clcalipso (npoints,lm) = lidarcld, cldlayer (npoints,4), cfad_sr (npoints,15,lm), parasolrefl
 * (npoints,5), lidarpmol (npoints,lm): the exports CLCALIPSO; CLLCALIPSO, CLMCALIPSO, CLHCALIPSO, CLTCALIPSO; CFADLIDARSR532_01 to _15;
 * PARASOLREFL0 (all five angles) and PARASOLREFL1 to PARASOLREFL5 (one each); LIDARPMOL (:3738-3750, :4204-4330).
 * The GridComp's rules around the call, oddities included: land = 1 where frocean < 0.5, else 0 (:3548, :3584); the lidar's presf is
 * ICARUS's phalf, presf(1) = 0, presf(k) = ple(k-2) (:3672 on PLECOSP(0:LM), cosp_lidar.F90:60-61): the surface pressure never enters and
 * the thickness of layer l is formed from the pressure difference of the layer above it; pplay is gbx%ph, the same edges, pplay(k) =
 * ple(k-1), not the mid-layer pressure (cosp_stats.F90:127); qltot and qitot are clamped at 0 (:3700); the convective contents and radii
 * are zero (:3687-3690).  The lidar reads the SCOPS mask this call made in the workspace; the mask never leaves HBM.
 * The five lidar outputs all NULL skips the lidar (frocean may then be NULL and ice_type is not looked at) and leaves every other bit as
 * geosrad_cosp_dev makes it.  ncol = 1 is what it is to geosrad_cosp_dev: GEOSRAD_EINVAL with a MISR output wanted, one sub-column a
 * point otherwise, for MODIS and the lidar alike.  Errors beside geosrad_cosp_dev's: with a lidar output wanted, frocean NULL or an
 * ice_type other than 0 or 1: GEOSRAD_EINVAL, before anything runs; the lidar's range check as for geosrad_lidar_dev. */
int geosrad_cosp_lidar_dev(geosrad_ctx *ctx, void *stream, int npoints, int lm, int ncol, const void *t, const void *qv, const void *fcld,
                           const void *cca, const void *ple, const void *plo, const void *dtau_s, const void *emiss, const void *dtau_c,
                           const void *dem_c, const void *ts, const int32_t *sunlit, int32_t *seed, int overlap, int top_height,
                           int top_height_direction, double emsfc_lw, void *fq_isccp, void *totalcldarea, void *meanptop,
                           void *meantaucld, void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau, void *boxptop, void *sgfcld,
                           const void *zle, const void *qltot, const void *qitot, const void *rdfl, const void *rdfi,
                           void *fq_MISR_TAU_v_CTH, void *dist_model_layertops, void *MISR_mean_ztop, void *MISR_cldarea, void *modis_mean,
                           void *modis_hist, const void *frocean, int ice_type, void *clcalipso, void *cldlayer, void *cfad_sr,
                           void *parasolrefl, void *lidarpmol);

#ifdef __cplusplus
}
#endif
#endif /* GEOSRAD_LIDAR_H */
