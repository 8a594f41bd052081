"""The fp32 tolerance policy of the suite, stated once (plain numpy, no GPU, no oracle import).

An fp32 evaluation is held to the oracle's own r4 - r8 spread on the same inputs, by quantile over the columns of a batch:

    e_dev[c] = max over levels / bands |dev32 - ref64| / scale[c]      the evaluation under test against the fp64 oracle
    e_ref[c] = max over levels / bands |ref32 - ref64| / scale[c]      what the oracle itself loses in fp32
    ratio_p  = Q_p(e_dev) / max(Q_p(e_ref), floor_p),   floor_p = floor_units * 2^-24 * Q_p(max |ref64| / scale)

and ratio_p <= 2 at p = 0.5 and 0.9, <= 4 at p = 0.99.

Why 2: dev32 and ref32 are two fp32 evaluations of the same formulae in different operation orders; their errors against fp64 have
the same size, so the evaluation under test may carry the oracle's error plus one more of the same.  Why 4 at 99 %: at 1024 columns
that quantile is decided by ten columns; under the oracle alone it moved by up to 1.34x between the two halves of a batch and by 4x
between batches of different seeds.  Why a floor: four units of fp32 round-off in the quantity's own size; a quantity the oracle gets
nearly exactly (the SW direct beam, 3e-8 of the TOA flux) would otherwise set a bound no other correct fp32 evaluation can meet.
These numbers are conditions of the policy, not fits to what any kernel gives.  The worst column is not judged here: it stays under
the worst-case bounds of the solvers' own tests (the PIFM singularity mu0 = 1/k decides it, not rounding in an ordinary column).

`scale` is per column: the column's TOA downward flux for RRTMG_SW, 1 for sorad (fractions of the insolation), 1 W m-2 for the LW
schemes.  Arrays carry the column on their last axis.

The two RRTMG solvers seed McICA from the pressure's fractional digits in the working precision, so the r4 and r8 oracles draw
different clouds and r4 - r8 says nothing about the total-sky fluxes of cloudy columns.  Those are compared with the r4 oracle
directly (`assert_direct_within_spread`), on the columns whose clearCounts agree, against the batch's clear-sky spread, at p = 0.5
and 0.9 only: a sub-column decision that flips without changing a count touches up to a few percent of the cloudy columns (flip rate
<= 2e-5 over about 2000 decisions a column), which moves the 99 % quantile and leaves the 90 % one alone."""
import numpy as np

QUANTILES = (0.5, 0.9, 0.99)
BOUND = {0.5: 2.0, 0.9: 2.0, 0.99: 4.0}
DIRECT_QUANTILES = (0.5, 0.9)
MIN_COLUMNS = 400          # below that the 99 % quantile is fewer than four columns
EPS32 = 2.0 ** -24


def _per_column(a, scale):
    """max over every axis but the last of |a|, over scale"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    ncol = a.shape[-1]
    return a.reshape(-1, ncol).max(axis=0) / np.broadcast_to(np.asarray(scale, dtype=np.float64), (ncol,))


def _f64(*arrays):
    out = [np.asarray(a, dtype=np.float64) for a in arrays]
    if len({a.shape for a in out}) != 1:
        raise ValueError(f"shapes differ: {[a.shape for a in out]}")
    if out[0].ndim < 1 or out[0].shape[-1] < MIN_COLUMNS:
        raise ValueError(f"a quantile of fewer than {MIN_COLUMNS} columns decides nothing: got shape {out[0].shape}")
    return out


def divergence(down, up):
    """flux divergence: the difference of the net flux between adjacent levels (what the tendencies kernel turns into heating)"""
    return np.diff(np.asarray(down, dtype=np.float64) - np.asarray(up, dtype=np.float64), axis=0)


def spread_ratios(dev32, ref32, ref64, scale, floor_units=4):
    """{p: dict(ratio, dev, ref, floor)} for p in QUANTILES; `dev` = Q_p(e_dev), `ref` = Q_p(e_ref) (module docstring)"""
    dev32, ref32, ref64 = _f64(dev32, ref32, ref64)
    e_dev = _per_column(dev32 - ref64, scale)
    e_ref = _per_column(ref32 - ref64, scale)
    size = _per_column(ref64, scale)
    out = {}
    for p in QUANTILES:
        q_dev, q_ref = float(np.quantile(e_dev, p)), float(np.quantile(e_ref, p))
        floor = floor_units * EPS32 * float(np.quantile(size, p))
        den = max(q_ref, floor)
        out[p] = dict(ratio=(q_dev / den if den > 0 else (0.0 if q_dev == 0 else np.inf)), dev=q_dev, ref=q_ref, floor=floor)
    return out


def format_ratios(name, r, ncol):
    return f"fp32-spread {name} [{ncol} columns]: " + "; ".join(
        f"p{100 * p:g} ratio {v['ratio']:.2f} (dev {v['dev']:.2e}, ref {v['ref']:.2e}, floor {v['floor']:.1e})" for p, v in r.items())


def assert_within_spread(name, dev32, ref32, ref64, scale, floor_units=4):
    """Prints every ratio with its two quantiles (pytest -s shows them), then asserts the bounds of the policy.  Returns the ratios."""
    r = spread_ratios(dev32, ref32, ref64, scale, floor_units)
    print(format_ratios(name, r, np.asarray(dev32).shape[-1]))
    over = {p: round(v["ratio"], 3) for p, v in r.items() if not v["ratio"] <= BOUND[p]}
    assert not over, f"{name}: fp32 error above the oracle's r4 - r8 spread, ratio by quantile {over} (bounds {BOUND})"
    return r


def direct_ratios(dev32, ref32, scale, ref_quantiles):
    """{p: dict(ratio, dev, ref)} for p in DIRECT_QUANTILES: Q_p(max |dev32 - ref32| / scale) over `ref_quantiles[p]`, the batch's clear-sky
    Q_p(e_ref) of the same quantity (spread_ratios(...)[p]['ref'])"""
    dev32, ref32 = _f64(dev32, ref32)
    e = _per_column(dev32 - ref32, scale)
    out = {}
    for p in DIRECT_QUANTILES:
        q, den = float(np.quantile(e, p)), float(ref_quantiles[p])
        out[p] = dict(ratio=(q / den if den > 0 else (0.0 if q == 0 else np.inf)), dev=q, ref=den)
    return out


def assert_direct_within_spread(name, dev32, ref32, scale, ref_quantiles):
    r = direct_ratios(dev32, ref32, scale, ref_quantiles)
    print(f"fp32-direct {name} [{np.asarray(dev32).shape[-1]} columns]: " + "; ".join(
        f"p{100 * p:g} ratio {v['ratio']:.2f} (dev - r4 {v['dev']:.2e}, clear-sky ref {v['ref']:.2e})" for p, v in r.items()))
    over = {p: round(v["ratio"], 3) for p, v in r.items() if not v["ratio"] <= BOUND[p]}
    assert not over, f"{name}: fp32 - r4 oracle above twice the batch's clear-sky r4 - r8 spread, ratio by quantile {over}"
    return r
