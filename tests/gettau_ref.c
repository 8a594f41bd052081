/* gettau_ref.c -- TEST INFRASTRUCTURE: the restatement of gettau.F90 (gettau_impl.h) on top of the oracle's Chou-Suarez SW and LW tables,
 * getvistau / getnirtau (cs_gettau) and getirtau (ch_getirtau), both precisions: gtr_swtau_f32 / _f64, gtr_irtau_*, gtr_oracle_swtau_*,
 * gtr_oracle_irtau_*, gtr_lw_cloud_diag_*, with the oracle's table setters alongside.  Built by tests/test_gettau_oracle.py into pytest's
 * temporary directory with -O2 -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define REAL float
#define SFX(x) x##_f32
#define EXP expf
#define LOG logf
#define POW powf
#define FMOD fmodf
#define FABS fabsf
#define SQRT sqrtf
#define LOG10 log10f
#define FLOOR floorf
#include "../oracle/lw_oracle_impl.h"
#include "../oracle/sw_oracle_impl.h"
#include "../oracle/chou_oracle_impl.h"
#include "../oracle/chou_sw_oracle_impl.h"
#include "../oracle/gridcomp_oracle_impl.h"
#include "gettau_impl.h"
#undef LOG10
#undef FLOOR
#undef NSOLFRAC
#undef REAL
#undef SFX
#undef EXP
#undef LOG
#undef POW
#undef FMOD
#undef FABS
#undef SQRT
#undef F2
#undef F3

#define REAL double
#define SFX(x) x##_f64
#define EXP exp
#define LOG log
#define POW pow
#define FMOD fmod
#define FABS fabs
#define SQRT sqrt
#define LOG10 log10
#define FLOOR floor
#include "../oracle/lw_oracle_impl.h"
#include "../oracle/sw_oracle_impl.h"
#include "../oracle/chou_oracle_impl.h"
#include "../oracle/chou_sw_oracle_impl.h"
#include "../oracle/gridcomp_oracle_impl.h"
#include "gettau_impl.h"
#undef LOG10
#undef FLOOR
#undef NSOLFRAC
#undef REAL
#undef SFX
#undef EXP
#undef LOG
#undef POW
#undef FMOD
#undef FABS
#undef SQRT
#undef F2
#undef F3
