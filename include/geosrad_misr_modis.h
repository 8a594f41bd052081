/* geosrad_misr_modis.h -- C ABI of the passive simulators of GEOSsatsim_GridComp's COSP beside ISCCP, as entry points of libgeosrad.so.
 * The fourth public header beside geosrad.h, geosrad_gettau.h and geosrad_satsim.h: same library, same geosrad_ctx, same conventions
 * (real_kind fixes the element type of every `const void *` / `void *` real array; arrays in the reference's Fortran layouts, the point
 * index the fastest; level 1 is the top of the atmosphere; any output may be NULL = not wanted; 0 or a GEOSRAD_E* code, the text from
 * geosrad_last_error).
 *
 *   geosrad_misr[_dev]       <- MISR_simulator.f:24-39                 (called at cosp_misr_simulator.F90:72-74)
 *   geosrad_modis[_dev]      <- the body of COSP_Modis_Simulator, cosp_modis_simulator.F90:69-296, with modis_simulator.F90
 *   geosrad_cosp_dev         <- call COSP with the ISCCP, MISR and MODIS simulators on: GEOS_SatsimGridComp.F90:3480-3510, :3722,
 *                               cosp_simulator.F90:113-126
 *
 * sunlit int32 (npoints): 1 day, anything else night.  zfull (m), at (K), dtau_s, dtau_c (npoints,nlev).  frac_out (npoints,ncol,nlev): the
 * SCOPS mask of geosrad_scops[_dev], 0 clear, 1 stratiform, 2 convective; the `_dev` variant holds it as one byte per cell, the host variant
 * in the real kind, which is what a Fortran caller holds.  fq_MISR_TAU_v_CTH (npoints,7 tau,16 heights; height 1 is "no height");
 * dist_model_layertops (npoints,16); MISR_mean_ztop, MISR_cldarea (npoints).
 *
 * The reference is reproduced statement by statement, with two things a caller may not expect:
 *   - the pattern matcher of MISR_simulator.f:314-335 reads and writes box_MISR_ztop(1,ibox): it adjusts the sub-columns of the FIRST POINT
 *     OF THE CALL only, sequentially in ibox; every other point is untouched;
 *   - a dark point (MISR_simulator.f:451-462) gets missing_value in fq_MISR_TAU_v_CTH, dist_model_layertops and MISR_cldarea, but the
 *     statement for the mean height sets MISR_mean_ztop(npoints): a dark point's MISR_mean_ztop stays 0, except that the LAST POINT OF THE
 *     CALL, if dark, gets missing_value.
 *   "First" and "last" are those of the call, not of a chunk of the host pipeline or of a shard of a geosrad_create_multi context.
 * Errors: npoints < 1, nlev < 2, ncol outside 2..65535, a null input: GEOSRAD_EINVAL.  ncol = 1 is refused because MISR_simulator.f:294-313
 * then couples neighbouring points in one serial scan over the grid, which is not a per-point computation.
 * The `_dev` variant takes device pointers and is asynchronous on `stream`; its workspace (two (npoints,ncol) planes) is taken at the first
 * call and counted by geosrad_workspace_bytes.  The host variant stages the arrays through the chunked pipeline of the solver entry points
 * (geosrad_set_chunk applies; chunks and the shards of a geosrad_create_multi context split the points only) and returns the `_dev` bits. */
#ifndef GEOSRAD_MISR_MODIS_H
#define GEOSRAD_MISR_MODIS_H

#include "geosrad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MISR_simulator.f:24-39  SUBROUTINE MISR_simulator(npoints,nlev,ncol,sunlit,zfull,at,dtau_s,dtau_c,frac_out,missing_value,
 * fq_MISR_TAU_v_CTH,dist_model_layertops,MISR_mean_ztop,MISR_cldarea) */
int geosrad_misr(geosrad_ctx *ctx, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *zfull, const void *at,
                 const void *dtau_s, const void *dtau_c, const void *frac_out, double missing_value, void *fq_MISR_TAU_v_CTH,
                 void *dist_model_layertops, void *MISR_mean_ztop, void *MISR_cldarea);
int geosrad_misr_dev(geosrad_ctx *ctx, void *stream, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *zfull,
                     const void *at, const void *dtau_s, const void *dtau_c, const void *frac_out_u8, double missing_value,
                     void *fq_MISR_TAU_v_CTH, void *dist_model_layertops, void *MISR_mean_ztop, void *MISR_cldarea);

/* modis_mean (npoints,17): the outputs of modis_L3_simulator in the order of its argument list, modis_simulator.F90:386-392 */
enum {
    GEOSRAD_MODIS_CF_TOTAL, GEOSRAD_MODIS_CF_WATER, GEOSRAD_MODIS_CF_ICE, GEOSRAD_MODIS_CF_HIGH, GEOSRAD_MODIS_CF_MID, GEOSRAD_MODIS_CF_LOW,
    GEOSRAD_MODIS_TAU_TOTAL, GEOSRAD_MODIS_TAU_WATER, GEOSRAD_MODIS_TAU_ICE, GEOSRAD_MODIS_LOGTAU_TOTAL, GEOSRAD_MODIS_LOGTAU_WATER,
    GEOSRAD_MODIS_LOGTAU_ICE, GEOSRAD_MODIS_SIZE_WATER, GEOSRAD_MODIS_SIZE_ICE, GEOSRAD_MODIS_CTP_TOTAL, GEOSRAD_MODIS_LWP, GEOSRAD_MODIS_IWP,
    GEOSRAD_MODIS_NMEAN
};

/* geosrad_modis[_dev]: the body of COSP_Modis_Simulator (cosp_modis_simulator.F90:69-296) on gridbox-level fields and the SCOPS mask, level 1
 * the top of the atmosphere.  t (K), p (Pa), dtau_s, dtau_c, the water contents mr_* and the radii reff_* (metres) (npoints,nlev); ph
 * (npoints,nlev+1) Pa, the layer edges from the top; isccp_boxtau, isccp_boxptop (npoints,ncol) from geosrad_icarus[_dev], the second in
 * hPa.  modis_simulator.F90:41-42 wants them from an ICARUS run with top_height = 1.  isccp_boxtau is accepted and not read: the reference
 * passes it and never uses it.  dtau_c and the four convective arrays may be NULL = zero.
 * What the reference does between these fields and modis_L2_simulator is done by index, without its five (npoints,ncol,nlev) arrays: a
 * cell's stratiform / convective fraction is the count of 1s / 2s in the mask over ncol; a stratiform cell of a sub-column carries
 * mr_lsliq / frac_ls, mr_lsice / frac_ls and the two ls radii, a convective one the cv ones over frac_cv, a clear one zeros; its optical
 * thickness is dtau_s, dtau_c or 0 (cosp.F90:414-431, :453-470, :484-494, cosp_modis_simulator.F90:146-170).  Then modis_L2_simulator_oneTau
 * and _twoTaus (modis_simulator.F90:361-375, :212-314) per sub-column, modis_L3_simulator (:445-527) per point and the wrapper's rules
 * (cosp_modis_simulator.F90:124-294): only points with sunlit > 0 are simulated; a dark point gets -1.0E30 (R_UNDEF) in all of modis_mean
 * and modis_hist and phase 0 / R_UNDEF in the L2 outputs.  modis_hist (npoints,7 tau,7 pressure): tau index 1 stays R_UNDEF (:338-339),
 * 2-7 hold the six bins from 0.3 (:229), the pressure index runs from the surface up (:233-234).  Cloud fractions are fractions, not
 * percent (the scaling of cosp_simulator.F90:177-206 hangs on flags GEOS_SatsimGridComp never sets).
 * Optional L2 results per sub-column (npoints,ncol): phase int32 (0 none, 1 liquid, 2 ice, 3 undetermined), ctp (Pa), tau, size (metres;
 * -999e-6 where the retrieval does not bracket the root).
 * Errors: npoints < 1, nlev < 2, ncol outside 1..65535, a null input: GEOSRAD_EINVAL.  Where modis_simulator.F90:202-206 calls
 * complain_and_die("Input values out of bounds") - on a sunlit point a temperature or layer pressure <= 0, a negative optical thickness or
 * a negative radius - the device sets a flag: the `_dev` variant reports it as GEOSRAD_EINPUT from geosrad_check with the array's name,
 * the host variant returns it.  Workspace: two (npoints,nlev) and four (npoints,ncol) planes. */
int geosrad_modis(geosrad_ctx *ctx, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *t, const void *p, const void *ph,
                  const void *dtau_s, const void *dtau_c, const void *frac_out, const void *mr_lsliq, const void *mr_lsice,
                  const void *mr_cvliq, const void *mr_cvice, const void *reff_lsliq, const void *reff_lsice, const void *reff_cvliq,
                  const void *reff_cvice, const void *isccp_boxtau, const void *isccp_boxptop, void *modis_mean, void *modis_hist,
                  int32_t *phase, void *ctp, void *tau, void *size);
int geosrad_modis_dev(geosrad_ctx *ctx, void *stream, int npoints, int nlev, int ncol, const int32_t *sunlit, const void *t, const void *p,
                      const void *ph, const void *dtau_s, const void *dtau_c, const void *frac_out_u8, const void *mr_lsliq,
                      const void *mr_lsice, const void *mr_cvliq, const void *mr_cvice, const void *reff_lsliq, const void *reff_lsice,
                      const void *reff_cvliq, const void *reff_cvice, const void *isccp_boxtau, const void *isccp_boxptop, void *modis_mean,
                      void *modis_hist, int32_t *phase, void *ctp, void *tau, void *size);

/* geosrad_cosp_dev: call COSP with the ISCCP, MISR and MODIS simulators on (GEOS_SatsimGridComp.F90:3480-3510, :3722,
 * cosp_simulator.F90:113-126), on GEOS fields in HBM, model order, nothing copied or flipped.  The arguments up to sgfcld are those of
 * geosrad_isccp_dev (geosrad_satsim.h), unchanged and in the same order, and the ISCCP outputs, the seeds and sgfcld are bit for bit that
 * entry point's.  Then zle (npoints,0:lm) m; qltot, qitot, rdfl, rdfi (npoints,lm); the four MISR outputs; modis_mean and modis_hist.
 * One SCOPS mask in the workspace serves the three simulators.  MISR's zfull(k) = 0.5 ((zle(k-1) - zle(lm)) + (zle(k) - zle(lm)))
 * (GEOS_SatsimGridComp.F90:3574-3580, :3696) and missing_value = R_UNDEF; MODIS's ph is ICARUS's phalf rule (ph(1) = 0, ph(k) = ple(k-2),
 * :3672, cosp_modis_simulator.F90:138-141), t and plo as they are, qltot and qitot clamped at 0 (:3700), the convective contents and radii
 * zero (:3687-3690, cosp_types.F90:1056, :1074).  MODIS reads the boxptop this call's ICARUS made with the caller's top_height:
 * modis_simulator.F90:41-42 wants top_height = 1.
 * An output group passed as all NULL skips that simulator (ISCCP: the nine of geosrad_icarus; SCOPS, the seeds and sgfcld are always
 * made); ISCCP still runs, into the workspace, when MODIS is wanted.  ncol = 1 with a MISR output wanted: GEOSRAD_EINVAL. */
int geosrad_cosp_dev(geosrad_ctx *ctx, void *stream, int npoints, int lm, int ncol, const void *t, const void *qv, const void *fcld,
                     const void *cca, const void *ple, const void *plo, const void *dtau_s, const void *emiss, const void *dtau_c,
                     const void *dem_c, const void *ts, const int32_t *sunlit, int32_t *seed, int overlap, int top_height,
                     int top_height_direction, double emsfc_lw, void *fq_isccp, void *totalcldarea, void *meanptop, void *meantaucld,
                     void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau, void *boxptop, void *sgfcld, const void *zle,
                     const void *qltot, const void *qitot, const void *rdfl, const void *rdfi, void *fq_MISR_TAU_v_CTH,
                     void *dist_model_layertops, void *MISR_mean_ztop, void *MISR_cldarea, void *modis_mean, void *modis_hist);

#ifdef __cplusplus
}
#endif
#endif /* GEOSRAD_MISR_MODIS_H */
