/* geosrad_gettau.h -- C ABI of the cloud optics of GEOS_RadiationShared/gettau.F90 as batched entry points of libgeosrad.so, and
 * the infrared cloud exports of LW_Driver for any longwave scheme.  A second public header beside geosrad.h: same library, same
 * geosrad_ctx, same conventions (real_kind fixes the element type of every `const void *` / `void *` real array; arrays in the
 * reference's Fortran layouts with the column index added in front as the fastest one; 0 or a GEOSRAD_E* code, the text from
 * geosrad_last_error).
 *
 *   geosrad_getvistau[_dev]  <- gettau::getvistau   GEOS_RadiationShared/gettau.F90:33-96   (body: getvistau.code)
 *   geosrad_getnirtau[_dev]  <- gettau::getnirtau   GEOS_RadiationShared/gettau.F90:102-167 (body: getnirtau.code)
 *   geosrad_getirtau[_dev]   <- gettau::getirtau    GEOS_RadiationShared/gettau.F90:173-224 (body: getirtau.code)
 *   geosrad_lw_cloud_diag_dev <- TAUIR / CLDTMP / CLDPRS of LW_Driver, GEOS_IrradGridComp.F90:1898-1912, :3626-3650
 *
 * The reference's routines take one column; these take ncol of them (callers: irrad.F90:645, sorad.F90:421-436, :955-968,
 * GEOS_SolarGridComp.F90:7266-7272, GEOS_SatsimGridComp.F90:3427-3431).
 *   cosz (ncol); dp, fcld (ncol,nlevs), dp in Pa; reff (ncol,nlevs,4) microns and hydromets (ncol,nlevs,4) kg/kg, species ice, liquid,
 *   rain, snow; grav: the caller's MAPL_GRAV (the routines `use MAPL_ConstantsMod, only: MAPL_GRAV`).
 *   ict = 0: the in-cloud mode (getvistau.code:7, :173-182) - the species' optical thicknesses as they are, icb is not read.
 *   ict /= 0: scaled for the maximum-random overlap of the super-layers above ict, from ict to icb - 1 and from icb down;
 *   1 <= ict <= icb <= nlevs + 1, an empty super-layer is legal (the reference's loops over it are empty).
 *   Outputs: taubeam, taudiff (ncol,nlevs,4); asycl, ssacl (ncol,nlevs); taudiag (ncol,nlevs,4); tcldlyr, enn (ncol,0:nlevs), level 0
 *   = 1 / 0 (getirtau.code:8-9).  An output may be NULL = not wanted: nothing is written there and nothing is computed for it; at
 *   least one must be given.  ib: the NIR band 1..3 (getnirtau) or the IR band 1..10 (getirtau).
 *   ncol <= 0, nlevs < 1, ib out of range, ict / icb outside the above, all outputs NULL: GEOSRAD_EINVAL.
 *   The Chou-Suarez SW tables (getvistau, getnirtau) or LW tables (getirtau, lw_cloud_diag) must have been loaded
 *   (geosrad_load_tables_chou_sw / geosrad_load_tables_chou_lw).
 * The `_dev` variants take device pointers and are asynchronous on `stream` (errors: geosrad_check).  The host variants stage the
 * arrays through the chunked pipeline of the solver entry points (geosrad_set_chunk applies; a geosrad_create_multi context cuts the
 * columns into one shard per device) and return the `_dev` results bit for bit. */
#ifndef GEOSRAD_GETTAU_H
#define GEOSRAD_GETTAU_H

#include "geosrad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gettau.F90:33-34  subroutine getvistau(nlevs,cosz,dp,fcld,reff,hydromets,ict,icb,taubeam,taudiff,asycl) */
int geosrad_getvistau(geosrad_ctx *ctx, int ncol, int nlevs, const void *cosz, const void *dp, const void *fcld, const void *reff,
                      const void *hydromets, int ict, int icb, double grav, void *taubeam, void *taudiff, void *asycl);
int geosrad_getvistau_dev(geosrad_ctx *ctx, void *stream, int ncol, int nlevs, const void *cosz, const void *dp, const void *fcld,
                          const void *reff, const void *hydromets, int ict, int icb, double grav, void *taubeam, void *taudiff,
                          void *asycl);

/* gettau.F90:102-103  subroutine getnirtau(ib,nlevs,cosz,dp,fcld,reff,hydromets,ict,icb,taubeam,taudiff,asycl,ssacl) */
int geosrad_getnirtau(geosrad_ctx *ctx, int ib, int ncol, int nlevs, const void *cosz, const void *dp, const void *fcld,
                      const void *reff, const void *hydromets, int ict, int icb, double grav, void *taubeam, void *taudiff,
                      void *asycl, void *ssacl);
int geosrad_getnirtau_dev(geosrad_ctx *ctx, void *stream, int ib, int ncol, int nlevs, const void *cosz, const void *dp,
                          const void *fcld, const void *reff, const void *hydromets, int ict, int icb, double grav, void *taubeam,
                          void *taudiff, void *asycl, void *ssacl);

/* gettau.F90:173-174  subroutine getirtau(ib,nlevs,dp,fcld,reff,hydromets,taudiag,tcldlyr,enn) */
int geosrad_getirtau(geosrad_ctx *ctx, int ib, int ncol, int nlevs, const void *dp, const void *fcld, const void *reff,
                     const void *hydromets, double grav, void *taudiag, void *tcldlyr, void *enn);
int geosrad_getirtau_dev(geosrad_ctx *ctx, void *stream, int ib, int ncol, int nlevs, const void *dp, const void *fcld,
                         const void *reff, const void *hydromets, double grav, void *taudiag, void *tcldlyr, void *enn);

/* geosrad_lw_cloud_diag_dev: the infrared cloud exports of LW_Driver from the GEOS fields in model ordering, whatever scheme computed
 * the fluxes.  In the reference's RRTMG branch TAUIR, CLDTMP and CLDPRS are formed from the local TAUDIAG (GEOS_IrradGridComp.F90:1516,
 * read at :3634-3650) that only `call IRRAD` fills (:2101): this entry point gives them there too.
 *   ple (ncol,0:lm) Pa; t, fcld, qi ql qr qs, ri rl rr rs (ncol,lm), radii in metres, `undef` (MAPL_UNDEF) allowed: 36 / 14 / 50 / 50
 *   microns then (:1905-1908); the fields are only read.  fcld does not enter these three exports and may be NULL.
 *   tauir (ncol,lm) = 0.5 (sum over species of getirtau's band 3 + of band 4); cldtmp, cldprs (ncol) = t(L), ple(L-1) of the first layer
 *   from the top with tauir(L) > taucrit / 2.13 (the division in the real kind, :3628), `undef` where there is none.  taucrit: the
 *   TAUCRIT: resource.  Each output may be NULL, at least one must be given; cldtmp needs t. */
int geosrad_lw_cloud_diag_dev(geosrad_ctx *ctx, void *stream, int ncol, int lm, double grav, double undef, double taucrit,
                              const void *ple, const void *t, const void *fcld, const void *qi, const void *ql, const void *qr,
                              const void *qs, const void *ri, const void *rl, const void *rr, const void *rs, void *tauir,
                              void *cldtmp, void *cldprs);

#ifdef __cplusplus
}
#endif
#endif /* GEOSRAD_GETTAU_H */
