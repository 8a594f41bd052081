/* geosrad_satsim.h -- C ABI of the ISCCP path of GEOSsatsim_GridComp as entry points of libgeosrad.so: the SCOPS sub-column generator,
 * the ICARUS ISCCP simulator and the COSP wrapper around them.  The third public header beside geosrad.h and geosrad_gettau.h: same
 * library, same geosrad_ctx, same conventions (real_kind fixes the element type of every `const void *` / `void *` real array; arrays in
 * the reference's Fortran layouts, the point index the fastest; 0 or a GEOSRAD_E* code, the text from geosrad_last_error).
 *
 *   geosrad_scops[_dev]      <- scops.f:1-2 with congvec.f             (called at cosp.F90:397)
 *   geosrad_icarus[_dev]     <- icarus.f:1-33                          (called at cosp_isccp_simulator.F90:74-80)
 *   geosrad_cosp_seeds_dev   <- cosp.F90:167-174
 *   geosrad_isccp_dev        <- call COSP with only the ISCCP simulator on: cosp.F90:167-174 is the caller's geosrad_cosp_seeds_dev, then
 *                               cosp.F90:392-397, :435, cosp_isccp_simulator.F90:58-90, GEOS_SatsimGridComp.F90:3727-3732
 *
 * Level 1 is the top of the atmosphere, as scops and icarus take their arrays (cosp.F90:392-393, cosp_isccp_simulator.F90:60-72) - which
 * is the GEOS model order.
 *   cc, conv, pfull, qv, dtau_s, dtau_c, at, dem_s, dem_c (npoints,nlev); phalf (npoints,nlev+1); skt (npoints); sunlit, seed int32 (npoints).
 *   frac_out (npoints,ncol,nlev): 0 clear, 1 stratiform, 2 convective.  The `_dev` variants hold it as one byte per cell, the host
 *   variants in the real kind, which is what a Fortran caller holds.
 *   seed: in/out, one Marsaglia CONG stream per point (congvec.f); SCOPS leaves the state after the last draw there.
 *   overlap 1 max, 2 random, 3 max/random; top_height 1, 2, 3 and top_height_direction 1, 2 as icarus.f:136-167.
 *   fq_isccp (npoints,7 tau,7 pressure); totalcldarea, meanptop, meantaucld, meanalbedocld, meantb, meantbclr (npoints); boxtau, boxptop
 *   (npoints,ncol); -1.E+30 where the reference leaves its missing value.  Any output may be NULL = not wanted.
 *   icarus.f's `debug`, `debugcol` and its printing are not part of the interface.
 * Errors: npoints < 1, nlev < 2, ncol outside 1..65535 (GEOS: Ncolumns <= 30; the histogram counts in 16 bits), overlap outside 1..3,
 * top_height outside 1..3, top_height_direction outside 1..2, a null input: GEOSRAD_EINVAL.  Where icarus.f:403-455 STOPs (cc, conv, dem_s, dem_c outside 0..1, a negative dtau_s, dtau_c) the device
 * sets a flag: the `_dev` variants report it as GEOSRAD_EINPUT from geosrad_check, the host variants return it.
 * The `_dev` variants take device pointers and are asynchronous on `stream`; their workspace (two (npoints,nlev) planes, four
 * (npoints,ncol) planes, for geosrad_isccp_dev the byte mask too) is taken at the first call and counted by geosrad_workspace_bytes.
 * The host variants stage the arrays through the chunked pipeline of the solver entry points (geosrad_set_chunk applies; chunks and the
 * shards of a geosrad_create_multi context split the points only - a point's stream never spans two) and return the `_dev` bits. */
#ifndef GEOSRAD_SATSIM_H
#define GEOSRAD_SATSIM_H

#include "geosrad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scops.f:1-2  subroutine scops(npoints,nlev,ncol,seed,cc,conv,overlap,frac_out,ncolprint) */
int geosrad_scops(geosrad_ctx *ctx, int npoints, int nlev, int ncol, int32_t *seed, const void *cc, const void *conv, int overlap,
                  void *frac_out);
int geosrad_scops_dev(geosrad_ctx *ctx, void *stream, int npoints, int nlev, int ncol, int32_t *seed, const void *cc, const void *conv,
                      int overlap, void *frac_out_u8);

/* icarus.f:1-33  SUBROUTINE ICARUS(debug,debugcol,npoints,sunlit,nlev,ncol,pfull,phalf,qv,cc,conv,dtau_s,dtau_c,top_height,
 * top_height_direction,overlap,frac_out,skt,emsfc_lw,at,dem_s,dem_c,fq_isccp,totalcldarea,meanptop,meantaucld,meanalbedocld,meantb,
 * meantbclr,boxtau,boxptop) */
int geosrad_icarus(geosrad_ctx *ctx, int npoints, const int32_t *sunlit, int nlev, int ncol, const void *pfull, const void *phalf,
                   const void *qv, const void *cc, const void *conv, const void *dtau_s, const void *dtau_c, int top_height,
                   int top_height_direction, int overlap, const void *frac_out, const void *skt, double emsfc_lw, const void *at,
                   const void *dem_s, const void *dem_c, void *fq_isccp, void *totalcldarea, void *meanptop, void *meantaucld,
                   void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau, void *boxptop);
int geosrad_icarus_dev(geosrad_ctx *ctx, void *stream, int npoints, const int32_t *sunlit, int nlev, int ncol, const void *pfull,
                       const void *phalf, const void *qv, const void *cc, const void *conv, const void *dtau_s, const void *dtau_c,
                       int top_height, int top_height_direction, int overlap, const void *frac_out_u8, const void *skt, double emsfc_lw,
                       const void *at, const void *dem_s, const void *dem_c, void *fq_isccp, void *totalcldarea, void *meanptop,
                       void *meantaucld, void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau, void *boxptop);

/* cosp.F90:167-174: seed = int((psfc - minval(psfc)) / (maxval(psfc) - minval(psfc)) * 100000) + 1 in the real kind over the call's
 * points; npoints = 1: int(psfc).  psfc real (npoints) - GEOS_SatsimGridComp.F90:3674 passes PLE(:,:,LM). */
int geosrad_cosp_seeds_dev(geosrad_ctx *ctx, void *stream, int npoints, const void *psfc, int32_t *seed);

/* geosrad_isccp_dev: the COSP ISCCP path on the fields as GEOS_SatsimGridComp holds them before it builds gbx (:3550-3568, :3665-3681),
 * model order, nothing copied or flipped.  t, qv, fcld, cca, plo, dtau_s, emiss, dtau_c, dem_c (npoints,lm); ple (npoints,0:lm) Pa; ts
 * (npoints).  dtau_s / emiss as geosrad_getvistau_dev / geosrad_getirtau_dev with ict = icb = 0 leave them summed over ice and liquid
 * (:3444-3452).  cca, dtau_c, dem_c may be NULL = zero (:3668-3678 sets the last two to zero).
 * What the reference does between these fields and icarus, done here by index: SCOPS on fcld, cca as they are (cosp.F90:392-397) with
 * `seed` (in/out); icarus' cc, conv = fcld, cca times 0.999999 (cosp_isccp_simulator.F90:65-66; icarus reads them in its range check only);
 * phalf(1) = 0, phalf(k) = ple(k-2) (:62-63 on gbx%ph = PLECOSP(:,1:LM), GEOS_SatsimGridComp.F90:3672);
 * ICARUS; fq_isccp(:,:,7:1:-1) and the snap of totalcldarea to 1 within 1.e-5 (:84-90).
 * sgfcld (npoints,lm), optional: GEOS_SatsimGridComp.F90:3727-3732.  boxtau, boxptop (npoints,ncol): what the MODIS simulator reads. */
int geosrad_isccp_dev(geosrad_ctx *ctx, void *stream, int npoints, int lm, int ncol, const void *t, const void *qv, const void *fcld,
                      const void *cca, const void *ple, const void *plo, const void *dtau_s, const void *emiss, const void *dtau_c,
                      const void *dem_c, const void *ts, const int32_t *sunlit, int32_t *seed, int overlap, int top_height,
                      int top_height_direction, double emsfc_lw, void *fq_isccp, void *totalcldarea, void *meanptop, void *meantaucld,
                      void *meanalbedocld, void *meantb, void *meantbclr, void *boxtau, void *boxptop, void *sgfcld);

#ifdef __cplusplus
}
#endif
#endif /* GEOSRAD_SATSIM_H */
