/* tests/sw_radval_ref.c -- TEST INFRASTRUCTURE ONLY.  The SOLAR_RADVAL restatement (tests/sw_radval_impl.h) on top of the oracle's
 * helpers, in both precisions; compiled by tests/test_sw_radval_oracle.py and tests/test_gpu_sw_radval.py into pytest's temporary
 * directory with the oracle's flags (gcc -O2 -ffp-contract=off -shared -fPIC). */
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
#include "sw_radval_impl.h"
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
#include "sw_radval_impl.h"
