// Host program of tests/test_field_tables.py: binds every Fields<S> table of csrc/gridcomp_kernels.hpp with a distinct pointer per slot of
// the public in[] / out[] tables and names, member by member, the slot each member must have received (the lists are the name-by-name
// statements the entry points made before the tables existed).  Prints the number of members checked; any mismatch ends it with status 1.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../geosradiation_gridcomp_amd/csrc/gridcomp_kernels.hpp"
using namespace geosrad;
using R = float;
static int checked = 0;
static void *slot(int k) { return (void *)(uintptr_t)(0x1000 + 8 * k); }
template <int N> struct Ptrs { const void *in[N]; void *out[N]; Ptrs() { for (int k = 0; k < N; k++) in[k] = out[k] = slot(k); } };
#define CK(member, K) do { checked++; if ((const void *)(member) != slot(K)) { fprintf(stderr, "%s != slot %s\n", #member, #K); exit(1); } } while (0)
#define NONE(member) do { checked++; if (member) { fprintf(stderr, "%s bound\n", #member); exit(1); } } while (0)

int main()
{
    Ptrs<64> P;
    { LwdArgs<R> A{}; bind_in<Fields<LwdArgs<R>>>(A, P.in);
      CK(A.ple, GEOSRAD_LWD_PLE); CK(A.pl, GEOSRAD_LWD_PL); CK(A.t, GEOSRAD_LWD_T); CK(A.q, GEOSRAD_LWD_Q); CK(A.o3, GEOSRAD_LWD_O3); CK(A.ch4, GEOSRAD_LWD_CH4);
      CK(A.n2o, GEOSRAD_LWD_N2O); CK(A.co2_3d, GEOSRAD_LWD_CO2_3D); CK(A.cfc11, GEOSRAD_LWD_CFC11); CK(A.cfc12, GEOSRAD_LWD_CFC12); CK(A.hcfc22, GEOSRAD_LWD_HCFC22);
      CK(A.fcld, GEOSRAD_LWD_FCLD); CK(A.cwc_liq, GEOSRAD_LWD_CWC_LIQ); CK(A.cwc_ice, GEOSRAD_LWD_CWC_ICE); CK(A.reff_liq, GEOSRAD_LWD_REFF_LIQ);
      CK(A.reff_ice, GEOSRAD_LWD_REFF_ICE); CK(A.taua, GEOSRAD_LWD_TAUA); CK(A.ssaa, GEOSRAD_LWD_SSAA); CK(A.ts, GEOSRAD_LWD_TS); CK(A.emis, GEOSRAD_LWD_EMIS);
      CK(A.lats, GEOSRAD_LWD_LATS); CK(A.t2m, GEOSRAD_LWD_T2M); NONE(A.play); NONE(A.alat); }
    { LwdPost<R> Q{}; bind_out<Fields<LwdPost<R>>>(Q, P.out);
      CK(Q.flxu_int, GEOSRAD_LWD_FLXU_INT); CK(Q.flxd_int, GEOSRAD_LWD_FLXD_INT); CK(Q.flcu_int, GEOSRAD_LWD_FLCU_INT); CK(Q.flcd_int, GEOSRAD_LWD_FLCD_INT);
      CK(Q.dfdts, GEOSRAD_LWD_DFDTS); CK(Q.dfdtsc, GEOSRAD_LWD_DFDTSC); CK(Q.dfdtsna, GEOSRAD_LWD_DFDTSNA); CK(Q.dfdtscna, GEOSRAD_LWD_DFDTSCNA);
      CK(Q.flx_int, GEOSRAD_LWD_FLX_INT); CK(Q.flc_int, GEOSRAD_LWD_FLC_INT); CK(Q.sfcem_int, GEOSRAD_LWD_SFCEM_INT); CK(Q.ts_int, GEOSRAD_LWD_TS_INT);
      CK(Q.cldttlw, GEOSRAD_LWD_CLDTTLW); CK(Q.cldhilw, GEOSRAD_LWD_CLDHILW); CK(Q.cldmdlw, GEOSRAD_LWD_CLDMDLW); CK(Q.cldlolw, GEOSRAD_LWD_CLDLOLW);
      NONE(Q.uflx); NONE(Q.emis); NONE(Q.ts); }
    { LwdRatPost<R> RP{}; bind_out<Fields<LwdRatPost<R>>>(RP, P.out);
      CK(RP.flxu_rat, GEOSRAD_LWD_FLXU_RAT); CK(RP.flxd_rat, GEOSRAD_LWD_FLXD_RAT); CK(RP.flx_rat, GEOSRAD_LWD_FLX_RAT); CK(RP.dfdts_rat, GEOSRAD_LWD_DFDTS_RAT);
      CK(RP.sfcem_rat, GEOSRAD_LWD_SFCEM_RAT); NONE(RP.uflx); NONE(RP.emis); }
    { LwRatUpd<R> U{}; bind(U, P.in, P.out);
      CK(U.flx_int, GEOSRAD_LWR_FLX_INT); CK(U.sfcem_int, GEOSRAD_LWR_SFCEM_INT); CK(U.dfdts, GEOSRAD_LWR_DFDTS); CK(U.flx_rat, GEOSRAD_LWR_FLX_RAT);
      CK(U.sfcem_rat, GEOSRAD_LWR_SFCEM_RAT); CK(U.dfdts_rat, GEOSRAD_LWR_DFDTS_RAT); CK(U.dolr, GEOSRAD_LWR_DOLR); CK(U.dlws, GEOSRAD_LWR_DLWS);
      CK(U.dflns, GEOSRAD_LWR_DFLNS); CK(U.dsfcem, GEOSRAD_LWR_DSFCEM); CK(U.nettrap, GEOSRAD_LWR_NETTRAP); CK(U.coltrap, GEOSRAD_LWR_COLTRAP);
      CK(U.flx, GEOSRAD_LWR_FLX); CK(U.dfdts_out, GEOSRAD_LWR_DFDTS_OUT); }
    { LwcPost<R> C{}; bind(C, P.in, P.out);
      CK(C.flxu, GEOSRAD_LWC_FLXU_INT); CK(C.flcu, GEOSRAD_LWC_FLCU_INT); CK(C.flau, GEOSRAD_LWC_FLAU_INT); CK(C.flxau, GEOSRAD_LWC_FLXAU_INT);
      CK(C.flxd, GEOSRAD_LWC_FLXD_INT); CK(C.flcd, GEOSRAD_LWC_FLCD_INT); CK(C.flad, GEOSRAD_LWC_FLAD_INT); CK(C.flxad, GEOSRAD_LWC_FLXAD_INT);
      CK(C.dfdts, GEOSRAD_LWC_DFDTS); CK(C.ts, GEOSRAD_LWC_TS); CK(C.sfcem_int, GEOSRAD_LWC_SFCEM_INT); CK(C.flx_int, GEOSRAD_LWC_FLX_INT);
      CK(C.flxa_int, GEOSRAD_LWC_FLXA_INT); CK(C.flc_int, GEOSRAD_LWC_FLC_INT); CK(C.fla_int, GEOSRAD_LWC_FLA_INT); CK(C.dfdtsc, GEOSRAD_LWC_DFDTSC);
      CK(C.dfdtsna, GEOSRAD_LWC_DFDTSNA); CK(C.dfdtscna, GEOSRAD_LWC_DFDTSCNA); CK(C.ts_int, GEOSRAD_LWC_TS_INT); }
    { SwcLit<R> L{}; bind_in<Fields<SwcLit<R>>>(L, P.in);
      CK(L.ple, GEOSRAD_SWC_PLE); CK(L.ox, GEOSRAD_SWC_OX); CK(L.lay_in[0], GEOSRAD_SWC_T); CK(L.lay_in[1], GEOSRAD_SWC_Q); CK(L.lay_in[2], GEOSRAD_SWC_CL);
      for (int s = 0; s < 4; s++) { CK(L.q[s], GEOSRAD_SWC_QI + s); CK(L.r[s], GEOSRAD_SWC_RI + s); }
      CK(L.aer_in[0], GEOSRAD_SWC_TAUA); CK(L.aer_in[1], GEOSRAD_SWC_SSAA); CK(L.aer_in[2], GEOSRAD_SWC_ASYA);
      CK(L.col_in[0], GEOSRAD_SWC_ZT); CK(L.col_in[1], GEOSRAD_SWC_ALBVR); CK(L.col_in[2], GEOSRAD_SWC_ALBVF); CK(L.col_in[3], GEOSRAD_SWC_ALBNR);
      CK(L.col_in[4], GEOSRAD_SWC_ALBNF); NONE(L.plhpa); NONE(L.lay_out[0]); NONE(L.lit); }
    { LwUpd<R> U{}; bind(U, P.in, P.out);
      CK(U.tsinst, GEOSRAD_LWU_TSINST); CK(U.ts_int, GEOSRAD_LWU_TS_INT); CK(U.sfcem_int, GEOSRAD_LWU_SFCEM_INT); CK(U.fcld, GEOSRAD_LWU_FCLD);
      CK(U.flx_int, GEOSRAD_LWU_FLX_INT); CK(U.flxa_int, GEOSRAD_LWU_FLXA_INT); CK(U.flc_int, GEOSRAD_LWU_FLC_INT); CK(U.fla_int, GEOSRAD_LWU_FLA_INT);
      CK(U.flxu_int, GEOSRAD_LWU_FLXU_INT); CK(U.flxau_int, GEOSRAD_LWU_FLXAU_INT); CK(U.flcu_int, GEOSRAD_LWU_FLCU_INT); CK(U.flau_int, GEOSRAD_LWU_FLAU_INT);
      CK(U.flxd_int, GEOSRAD_LWU_FLXD_INT); CK(U.flxad_int, GEOSRAD_LWU_FLXAD_INT); CK(U.flcd_int, GEOSRAD_LWU_FLCD_INT); CK(U.flad_int, GEOSRAD_LWU_FLAD_INT);
      CK(U.dfdts, GEOSRAD_LWU_DFDTS); CK(U.dfdtsna, GEOSRAD_LWU_DFDTSNA); CK(U.dfdtsc, GEOSRAD_LWU_DFDTSC); CK(U.dfdtscna, GEOSRAD_LWU_DFDTSCNA);
      CK(U.flx, GEOSRAD_LWU_FLX); CK(U.flxa, GEOSRAD_LWU_FLXA); CK(U.flc, GEOSRAD_LWU_FLC); CK(U.fla, GEOSRAD_LWU_FLA); CK(U.flxu, GEOSRAD_LWU_FLXU);
      CK(U.flxau, GEOSRAD_LWU_FLXAU); CK(U.flcu, GEOSRAD_LWU_FLCU); CK(U.flau, GEOSRAD_LWU_FLAU); CK(U.flxd, GEOSRAD_LWU_FLXD); CK(U.flxad, GEOSRAD_LWU_FLXAD);
      CK(U.flcd, GEOSRAD_LWU_FLCD); CK(U.flad, GEOSRAD_LWU_FLAD); CK(U.olr, GEOSRAD_LWU_OLR); CK(U.olra, GEOSRAD_LWU_OLRA); CK(U.olc, GEOSRAD_LWU_OLC);
      CK(U.ola, GEOSRAD_LWU_OLA); CK(U.olcc5, GEOSRAD_LWU_OLCC5); CK(U.dsfdts, GEOSRAD_LWU_DSFDTS); CK(U.sfcem, GEOSRAD_LWU_SFCEM); CK(U.lws, GEOSRAD_LWU_LWS);
      CK(U.lwsa, GEOSRAD_LWU_LWSA); CK(U.lcs, GEOSRAD_LWU_LCS); CK(U.las, GEOSRAD_LWU_LAS); CK(U.lcsc5, GEOSRAD_LWU_LCSC5); CK(U.flns, GEOSRAD_LWU_FLNS);
      CK(U.flnsna, GEOSRAD_LWU_FLNSNA); CK(U.flnsc, GEOSRAD_LWU_FLNSC); CK(U.flnsa, GEOSRAD_LWU_FLNSA); CK(U.dsfdts0, GEOSRAD_LWU_DSFDTS0);
      CK(U.sfcem0, GEOSRAD_LWU_SFCEM0); CK(U.tsreff, GEOSRAD_LWU_TSREFF); CK(U.cldtt, GEOSRAD_LWU_CLDTT); }
    { LwkSurf<R> S{}; bind_in<Fields<LwkSurf<R>>>(S, P.in);
      CK(S.ple, GEOSRAD_LWK_PLE); CK(S.t, GEOSRAD_LWK_T); CK(S.ts, GEOSRAD_LWK_TS); CK(S.emis, GEOSRAD_LWK_EMIS); NONE(S.t2m); NONE(S.rv); }
    { LwkDiag<R> D{}; bind(D, P.in, P.out);
      CK(D.t, GEOSRAD_LWK_T); CK(D.ple, GEOSRAD_LWK_PLE); CK(D.ts, GEOSRAD_LWK_TS); CK(D.dfdts, GEOSRAD_LWK_DFDTS); CK(D.sfcem_int, GEOSRAD_LWK_SFCEM_INT);
      CK(D.flx_int, GEOSRAD_LWK_FLX_INT); CK(D.tauir, GEOSRAD_LWK_TAUIR); CK(D.cldtmp, GEOSRAD_LWK_CLDTMP); CK(D.cldprs, GEOSRAD_LWK_CLDPRS);
      CK(D.tsreff, GEOSRAD_LWK_TSREFF); CK(D.dsfdts0, GEOSRAD_LWK_DSFDTS0); CK(D.sfcem0, GEOSRAD_LWK_SFCEM0); CK(D.lws0, GEOSRAD_LWK_LWS0); NONE(D.taudiag); }
    { SwdLit<R> A{}; bind_in<Fields<SwdLit<R>>>(A, P.in);
      CK(A.ple, GEOSRAD_SWD_PLE); CK(A.pl, GEOSRAD_SWD_PL); CK(A.t, GEOSRAD_SWD_T); CK(A.q, GEOSRAD_SWD_Q); CK(A.o3, GEOSRAD_SWD_O3); CK(A.ch4, GEOSRAD_SWD_CH4);
      CK(A.cl, GEOSRAD_SWD_CL); CK(A.ts, GEOSRAD_SWD_TS); CK(A.qq_ice, GEOSRAD_SWD_QQ_ICE); CK(A.qq_liq, GEOSRAD_SWD_QQ_LIQ); CK(A.rr_ice, GEOSRAD_SWD_RR_ICE);
      CK(A.rr_liq, GEOSRAD_SWD_RR_LIQ); CK(A.taua, GEOSRAD_SWD_TAUA); CK(A.ssaa, GEOSRAD_SWD_SSAA); CK(A.asya, GEOSRAD_SWD_ASYA);
      CK(A.col_in[0], GEOSRAD_SWD_ZT); CK(A.col_in[1], GEOSRAD_SWD_ALAT); CK(A.col_in[2], GEOSRAD_SWD_ALBVR); CK(A.col_in[3], GEOSRAD_SWD_ALBVF);
      CK(A.col_in[4], GEOSRAD_SWD_ALBNR); CK(A.col_in[5], GEOSRAD_SWD_ALBNF); NONE(A.play); NONE(A.col_out[0]); NONE(A.lit); }
    { SwdPost<R> Q{}; bind_out<Fields<SwdPost<R>>>(Q, P.out);
      CK(Q.fsw, GEOSRAD_SWD_FSW); CK(Q.fsc, GEOSRAD_SWD_FSC); CK(Q.fswu, GEOSRAD_SWD_FSWU); CK(Q.fscu, GEOSRAD_SWD_FSCU); CK(Q.cldts, GEOSRAD_SWD_CLDTS);
      CK(Q.cldhs, GEOSRAD_SWD_CLDHS); CK(Q.cldms, GEOSRAD_SWD_CLDMS); CK(Q.cldls, GEOSRAD_SWD_CLDLS);
      for (int k = 0; k < 4; k++) { CK(Q.cot[k], GEOSRAD_SWD_COTTP + k); NONE(Q.cotn[k]); NONE(Q.cotd[k]); }
      NONE(Q.swuflx); }
    { SwdPost<R> N{}; bind_out<SwdPostNa<R>>(N, P.out);
      CK(N.fsw, GEOSRAD_SWD_FSWNA); CK(N.fsc, GEOSRAD_SWD_FSCNA); CK(N.fswu, GEOSRAD_SWD_FSWUNA); CK(N.fscu, GEOSRAD_SWD_FSCUNA);
      NONE(N.cldts); NONE(N.cldhs); NONE(N.cldms); NONE(N.cldls); for (int k = 0; k < 4; k++) NONE(N.cot[k]); }
    { SwSfc<R> U{}; bind(U, P.in, P.out);
      CK(U.slr, GEOSRAD_SWS_SLR); CK(U.zth, GEOSRAD_SWS_ZTH); CK(U.fswn, GEOSRAD_SWS_FSWN); CK(U.fscn, GEOSRAD_SWS_FSCN); CK(U.fswnan, GEOSRAD_SWS_FSWNAN);
      CK(U.fscnan, GEOSRAD_SWS_FSCNAN); CK(U.albedo, GEOSRAD_SWS_ALBEDO); CK(U.slrtp, GEOSRAD_SWS_SLRTP);
      for (int k = 0; k < 4; k++) { CK(U.alb_imp[k], GEOSRAD_SWS_ALBVF + k); CK(U.alb_exp[k], GEOSRAD_SWS_ALBVF_X + k); }
      for (int k = 0; k < 6; k++) { CK(U.dn[k], GEOSRAD_SWS_DRUVRN + k); CK(U.dx[k], GEOSRAD_SWS_DRUVR + k); }
      for (int k = 0; k < 3; k++) CK(U.drn[k], GEOSRAD_SWS_DRNUVR + k);
      CK(U.slrsf, GEOSRAD_SWS_SLRSF); CK(U.slrsfc, GEOSRAD_SWS_SLRSFC); CK(U.slrsfna, GEOSRAD_SWS_SLRSFNA); CK(U.slrsfcna, GEOSRAD_SWS_SLRSFCNA);
      CK(U.slrsuf, GEOSRAD_SWS_SLRSUF); CK(U.slrsufc, GEOSRAD_SWS_SLRSUFC); CK(U.slrsufna, GEOSRAD_SWS_SLRSUFNA); CK(U.slrsufcna, GEOSRAD_SWS_SLRSUFCNA); }
    { SwUpd<R> U{}; bind(U, P.in, P.out);
      CK(U.slr, GEOSRAD_SWU_SLR); CK(U.fswn, GEOSRAD_SWU_FSWN); CK(U.fscn, GEOSRAD_SWU_FSCN); CK(U.fswnan, GEOSRAD_SWU_FSWNAN); CK(U.fscnan, GEOSRAD_SWU_FSCNAN);
      CK(U.fswun, GEOSRAD_SWU_FSWUN); CK(U.fscun, GEOSRAD_SWU_FSCUN); CK(U.fswunan, GEOSRAD_SWU_FSWUNAN); CK(U.fscunan, GEOSRAD_SWU_FSCUNAN);
      CK(U.fswbandn, GEOSRAD_SWU_FSWBANDN); CK(U.fswbandnan, GEOSRAD_SWU_FSWBANDNAN);
      CK(U.fsw, GEOSRAD_SWU_FSW); CK(U.fsc, GEOSRAD_SWU_FSC); CK(U.fswna, GEOSRAD_SWU_FSWNA); CK(U.fscna, GEOSRAD_SWU_FSCNA); CK(U.fswu, GEOSRAD_SWU_FSWU);
      CK(U.fscu, GEOSRAD_SWU_FSCU); CK(U.fswuna, GEOSRAD_SWU_FSWUNA); CK(U.fscuna, GEOSRAD_SWU_FSCUNA); CK(U.fswd, GEOSRAD_SWU_FSWD); CK(U.fscd, GEOSRAD_SWU_FSCD);
      CK(U.fswdna, GEOSRAD_SWU_FSWDNA); CK(U.fscdna, GEOSRAD_SWU_FSCDNA); CK(U.fswband, GEOSRAD_SWU_FSWBAND); CK(U.fswbandna, GEOSRAD_SWU_FSWBANDNA);
      CK(U.rsr, GEOSRAD_SWU_RSR); CK(U.rsc, GEOSRAD_SWU_RSC); CK(U.rsrna, GEOSRAD_SWU_RSRNA); CK(U.rscna, GEOSRAD_SWU_RSCNA); CK(U.rsrs, GEOSRAD_SWU_RSRS);
      CK(U.rscs, GEOSRAD_SWU_RSCS); CK(U.rsrsna, GEOSRAD_SWU_RSRSNA); CK(U.rscsna, GEOSRAD_SWU_RSCSNA); CK(U.osr, GEOSRAD_SWU_OSR);
      CK(U.osrclr, GEOSRAD_SWU_OSRCLR); CK(U.osrna, GEOSRAD_SWU_OSRNA); CK(U.osrcna, GEOSRAD_SWU_OSRCNA); }
    { RadTend<R> T{}; bind(T, P.in, P.out);
      CK(T.ple, GEOSRAD_RT_PLE); CK(T.flw, GEOSRAD_RT_FLW); CK(T.fsw, GEOSRAD_RT_FSW); CK(T.flwclr, GEOSRAD_RT_FLWCLR); CK(T.fswclr, GEOSRAD_RT_FSWCLR);
      CK(T.fswna, GEOSRAD_RT_FSWNA); CK(T.fla, GEOSRAD_RT_FLA); CK(T.fscna, GEOSRAD_RT_FSCNA); CK(T.dsfdts, GEOSRAD_RT_DSFDTS); CK(T.sfcem, GEOSRAD_RT_SFCEM);
      CK(T.trd, GEOSRAD_RT_TRD); CK(T.dtdt, GEOSRAD_RT_DTDT); CK(T.radlw, GEOSRAD_RT_RADLW); CK(T.radsw, GEOSRAD_RT_RADSW); CK(T.radlwc, GEOSRAD_RT_RADLWC);
      CK(T.radswc, GEOSRAD_RT_RADSWC); CK(T.radswna, GEOSRAD_RT_RADSWNA); CK(T.radlwcna, GEOSRAD_RT_RADLWCNA); CK(T.radswcna, GEOSRAD_RT_RADSWCNA);
      CK(T.blw, GEOSRAD_RT_BLW); CK(T.alw, GEOSRAD_RT_ALW); CK(T.radsrf, GEOSRAD_RT_RADSRF); }
    printf("%d members checked\n", checked);
    return 0;
}
