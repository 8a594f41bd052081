"""numpy restatement of the SOLAR TO OBIO conversion of UPDATE_EXPORT (GEOSsolar_GridComp/GEOS_SolarGridComp.F90:7584-7737), written
from the Fortran: the band tables (:6794-6847, rrtmg_sw_init.F90:187-190), the walk over the solver's and the 33 OBIO bands in increasing
wavenumber (:7665-7728) and the accumulate-then-scale step (:7666-7667, :7719-7720, :7731-7734).  Every operation is made on numpy
scalars / arrays of the given dtype (float32 | float64), which round each operation like the compiled statements without contraction."""
import numpy as np

NB_OBIO = 33

# OBIO bands (start, finish) in [nm] (:6794-6829)
OBIO_BANDS_NM = [(200.0, 300.0), (300.0, 350.0), (350.0, 362.5), (362.5, 387.5), (387.5, 412.5), (412.5, 437.5), (437.5, 462.5),
                 (462.5, 487.5), (487.5, 512.5), (512.5, 537.5), (537.5, 562.5), (562.5, 587.5), (587.5, 612.5), (612.5, 637.5),
                 (637.5, 662.5), (662.5, 687.5), (687.5, 700.0), (700.0, 750.0), (750.0, 800.0), (800.0, 900.0), (900.0, 1000.0),
                 (1000.0, 1100.0), (1100.0, 1200.0), (1200.0, 1300.0), (1300.0, 1400.0), (1400.0, 1500.0), (1500.0, 1600.0),
                 (1600.0, 1700.0), (1700.0, 1800.0), (1800.0, 2000.0), (2000.0, 2400.0), (2400.0, 3400.0), (3400.0, 4000.0)]
# CHOU bands (start, finish) in [nm] (:6838-6847)
CHOU_BANDS_NM = [(225.0, 285.0), (285.0, 300.0), (300.0, 325.0), (325.0, 400.0), (400.0, 690.0), (690.0, 1220.0), (1220.0, 2270.0),
                 (2270.0, 3850.0)]
# rrsw_wvn wavenum1 / wavenum2 (16:29) (rrtmg_sw_init.F90:187-190)
RRTMG_WAVENUM1 = [2600., 3250., 4000., 4650., 5150., 6150., 7700., 8050., 12850., 16000., 22650., 29000., 38000., 820.]
RRTMG_WAVENUM2 = [3250., 4000., 4650., 5150., 6150., 7700., 8050., 12850., 16000., 22650., 29000., 38000., 50000., 2600.]


class BandsError(Exception):
    """a failed _ASSERT of the walk; str() is the reference's text"""


def solar_bands(scheme, dtype):
    """(wvn1, wvn2, order): limits [cm-1] in dtype and SOLAR_band_number_in_wvn_order (1-based)"""
    dt = np.dtype(dtype).type
    if scheme == "RRTMG":                                   # :7636-7644
        return [dt(x) for x in RRTMG_WAVENUM1], [dt(x) for x in RRTMG_WAVENUM2], [14] + list(range(1, 14))
    if scheme == "CHOU":                                    # :7655-7659
        return [dt(1.e7) / dt(b) for a, b in CHOU_BANDS_NM], [dt(1.e7) / dt(a) for a, b in CHOU_BANDS_NM], list(range(8, 0, -1))
    raise ValueError(scheme)


def walk(wvn1, wvn2, order, dtype):
    """the list of (ib, kb, sfrac) (1-based band numbers) in the order the reference accumulates them (:7665-7728)"""
    dt = np.dtype(dtype).type
    swv = [(dt(a), dt(b)) for a, b in zip(wvn1, wvn2)]
    owv = [(dt(1.e7) / dt(b), dt(1.e7) / dt(a)) for a, b in OBIO_BANDS_NM]      # 1.e7 / OBIO_bands_nm(2:1:-1,:)
    pairs = []
    sfirst = ofirst = True
    kb_start = NB_OBIO
    kb_used_last = None
    swvn2 = owvn2 = None
    for jb in range(1, len(order) + 1):
        ib = order[jb - 1]
        swvn1 = swv[ib - 1][0]
        if not sfirst and not swvn1 == swvn2:
            raise BandsError("SOLAR bands not complete and unique!")
        swvn2 = swv[ib - 1][1]
        sfirst = False
        for kb in range(kb_start, 0, -1):
            owvn1 = owv[kb - 1][0]
            if not ofirst and kb != kb_used_last and not owvn1 == owvn2:
                raise BandsError("OBIO bands not complete and unique!")
            owvn2 = owv[kb - 1][1]
            kb_used_last = kb
            ofirst = False
            kb_start = kb
            if owvn1 >= swvn2:
                break
            if owvn2 <= swvn1:
                continue
            sfrac = (min(swvn2, owvn2) - max(swvn1, owvn1)) / (swvn2 - swvn1)
            assert type(sfrac) is dt
            pairs.append((ib, kb, sfrac))
            if owvn2 > swvn2:
                break
    return pairs


def weights(pairs, nbands):
    """(nbands, 33) float64 = the C ABI's `weights`, widened"""
    w = np.zeros((nbands, NB_OBIO), dtype=np.float64)
    for ib, kb, sfrac in pairs:
        w[ib - 1, kb - 1] = float(sfrac)
    return w


def convert(pairs, xbandn, slr, dtype):
    """DROBIO (33, ncol) from DRBANDN (nbands, ncol) and SLR (ncol): zero, accumulate pair by pair, unnormalise (:7666-7734)"""
    x = np.asarray(xbandn, dtype=dtype)
    s = np.asarray(slr, dtype=dtype)
    out = np.zeros((NB_OBIO, x.shape[1]), dtype=dtype)
    for ib, kb, sfrac in pairs:
        out[kb - 1] = out[kb - 1] + x[ib - 1] * sfrac
    for kb in range(NB_OBIO):
        out[kb] = out[kb] * s
    return out
