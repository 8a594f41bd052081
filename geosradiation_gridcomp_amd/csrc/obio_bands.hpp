// obio_bands.hpp -- the band bookkeeping of UPDATE_EXPORT's SOLAR TO OBIO conversion (GEOSsolar_GridComp/GEOS_SolarGridComp.F90:7584-7737)
// on the host: the 33 ocean-biology bands (OBIO_bands_nm, :6794-6835), the solver's bands (rrsw_wvn's wavenum1/2(16:29) for RRTMG,
// :7636-7648; CHOU_bands_nm for Chou-Suarez, :6838-6847, :7652-7661) and the walk over both in increasing wavenumber (:7665-7728) that
// yields, for every overlapping (solar band, OBIO band) pair, the fraction `sfrac` of the solar band's wavenumber interval inside the
// OBIO band.  Every operation is made in T (float | double = the reference built with real*4 | -r8).  No device code here.
#pragma once
#include <cstdint>
#include "../../include/geosrad.h"

namespace geosrad {

constexpr int NB_OBIO = GEOSRAD_NB_OBIO;
constexpr int OBIO_MAXBANDS = GEOSRAD_OBIO_MAXBANDS;          // solar bands a caller of GEOSRAD_OBIO_BANDS may hand over
constexpr int OBIO_MAXPAIRS = OBIO_MAXBANDS + NB_OBIO - 1;    // two gapless partitions walked together overlap at most nb + 33 - 1 times

// OBIO bands (start, finish) in nm (:6794-6835)
static const float OBIO_BANDS_NM[NB_OBIO][2] = {
    {200.0f, 300.0f}, {300.0f, 350.0f}, {350.0f, 362.5f}, {362.5f, 387.5f}, {387.5f, 412.5f}, {412.5f, 437.5f}, {437.5f, 462.5f},
    {462.5f, 487.5f}, {487.5f, 512.5f}, {512.5f, 537.5f}, {537.5f, 562.5f}, {562.5f, 587.5f}, {587.5f, 612.5f}, {612.5f, 637.5f},
    {637.5f, 662.5f}, {662.5f, 687.5f}, {687.5f, 700.0f}, {700.0f, 750.0f}, {750.0f, 800.0f}, {800.0f, 900.0f}, {900.0f, 1000.0f},
    {1000.0f, 1100.0f}, {1100.0f, 1200.0f}, {1200.0f, 1300.0f}, {1300.0f, 1400.0f}, {1400.0f, 1500.0f}, {1500.0f, 1600.0f},
    {1600.0f, 1700.0f}, {1700.0f, 1800.0f}, {1800.0f, 2000.0f}, {2000.0f, 2400.0f}, {2400.0f, 3400.0f}, {3400.0f, 4000.0f}};
// Chou-Suarez bands (start, finish) in nm, band 2 = sub-band 2b (:6838-6847)
static const float CHOU_BANDS_NM[8][2] = {{225.0f, 285.0f}, {285.0f, 300.0f}, {300.0f, 325.0f}, {325.0f, 400.0f}, {400.0f, 690.0f},
                                          {690.0f, 1220.0f}, {1220.0f, 2270.0f}, {2270.0f, 3850.0f}};
// rrsw_wvn: wavenum1 / wavenum2 (jpb1:jpb2 = 16:29) in cm-1 (rrtmg_sw_init.F90:187-190); band 14 is out of order
static const float RRTMG_SW_WAVENUM1[14] = {2600.f, 3250.f, 4000.f, 4650.f, 5150.f, 6150.f, 7700.f, 8050.f, 12850.f, 16000.f, 22650.f, 29000.f, 38000.f, 820.f};
static const float RRTMG_SW_WAVENUM2[14] = {3250.f, 4000.f, 4650.f, 5150.f, 6150.f, 7700.f, 8050.f, 12850.f, 16000.f, 22650.f, 29000.f, 38000.f, 50000.f, 2600.f};

// The solar bands of `scheme` in T: limits in cm-1 and the 1-based band numbers in increasing wavenumber.  Null = fine, else the complaint.
template <typename T>
const char *obio_solar_bands(int scheme, int nbands, const double *wvn1, const double *wvn2, const int32_t *order, T *s1, T *s2, int *ord)
{
    if (scheme == GEOSRAD_OBIO_RRTMG) {
        if (nbands != 14) return "wrong number of RRTMG bands!";                              // :7633
        for (int i = 0; i < 14; i++) { s1[i] = (T)RRTMG_SW_WAVENUM1[i]; s2[i] = (T)RRTMG_SW_WAVENUM2[i]; }
        ord[0] = 14;                                                                          // :7643-7644
        for (int i = 1; i < 14; i++) ord[i] = i;
    } else if (scheme == GEOSRAD_OBIO_CHOU) {
        if (nbands != 8) return "wrong number of Chou-Suarez bands (8)";
        for (int i = 0; i < 8; i++) { s1[i] = (T)1.e7f / (T)CHOU_BANDS_NM[i][1]; s2[i] = (T)1.e7f / (T)CHOU_BANDS_NM[i][0]; }      // :7655-7656
        for (int i = 0; i < 8; i++) ord[i] = 8 - i;                                           // :7659
    } else if (scheme == GEOSRAD_OBIO_BANDS) {
        if (nbands < 1 || nbands > OBIO_MAXBANDS) return "nbands must lie in 1 .. GEOSRAD_OBIO_MAXBANDS";
        if (!wvn1 || !wvn2 || !order) return "wvn1 / wvn2 / order null";
        bool seen[OBIO_MAXBANDS] = {};
        for (int i = 0; i < nbands; i++) {
            s1[i] = (T)wvn1[i]; s2[i] = (T)wvn2[i];
            if (!(s1[i] < s2[i])) return "band limits must satisfy wvn1 < wvn2";
            if (order[i] < 1 || order[i] > nbands || seen[order[i] - 1]) return "order is not a permutation of 1 .. nbands";
            seen[order[i] - 1] = true;
            ord[i] = order[i];
        }
    } else return "scheme must be GEOSRAD_OBIO_CHOU, _RRTMG or _BANDS";
    return nullptr;
}

// :7665-7728, statement by statement; pair(jb, ib, kb, sfrac) (jb: 0-based position in wavenumber order; ib, kb: 1-based band numbers) stands
// for `DROBIO(:,:,kb) = DROBIO(:,:,kb) + DRBANDN(:,:,ib) * sfrac`.  Null = fine, else the text of the reference's failed _ASSERT.
template <typename T, typename F> const char *obio_walk(int nbands, const T *s1, const T *s2, const int *ord, F &&pair)
{
    T OW[NB_OBIO][2];                                         // OBIO_bands_wavenum = 1.e7 / OBIO_bands_nm(2:1:-1,:)
    for (int k = 0; k < NB_OBIO; k++) { OW[k][0] = (T)1.e7f / (T)OBIO_BANDS_NM[k][1]; OW[k][1] = (T)1.e7f / (T)OBIO_BANDS_NM[k][0]; }
    bool sfirst = true, ofirst = true;
    int kb_start = NB_OBIO, kb_used_last = 0;
    T swvn1, swvn2 = 0, owvn1, owvn2 = 0;
    for (int jb = 1; jb <= nbands; jb++) {
        const int ib = ord[jb - 1];
        swvn1 = s1[ib - 1];
        if (!sfirst && !(swvn1 == swvn2)) return "SOLAR bands not complete and unique!";
        swvn2 = s2[ib - 1];
        sfirst = false;
        for (int kb = kb_start; kb >= 1; kb--) {
            owvn1 = OW[kb - 1][0];
            if (!ofirst && kb != kb_used_last && !(owvn1 == owvn2)) return "OBIO bands not complete and unique!";
            owvn2 = OW[kb - 1][1];
            kb_used_last = kb;
            ofirst = false;
            kb_start = kb;
            if (owvn1 >= swvn2) break;
            if (owvn2 <= swvn1) continue;
            const T lo = swvn1 > owvn1 ? swvn1 : owvn1, hi = swvn2 < owvn2 ? swvn2 : owvn2;      // max(swvn1,owvn1), min(swvn2,owvn2)
            const T sfrac = (hi - lo) / (swvn2 - swvn1);
            pair(jb - 1, ib, kb, sfrac);
            if (owvn2 > swvn2) break;
        }
    }
    return nullptr;
}

}  // namespace geosrad
