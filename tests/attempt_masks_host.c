/* Stand-alone host program over the host twins of the mask helpers of a step attempt's tail (pgr_mask_lt_const,
 * pgr_mask_reached, pgr_factor_limit, pgr_step_factor, pgr_lane_pending: pygenray_amd/csrc/pgr_crmath.h with PGR_CR_HOST)
 * -- TEST INFRASTRUCTURE ONLY, CPU build:
 *   gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=gnu99 -ffp-contract=off \
 *       tests/attempt_masks_host.c -lm -o attempt_masks_host && ./attempt_masks_host
 * Every mask predicate against the plain comparison it replaces, bit for bit, on the doubles next to each threshold (1,
 * MAX_FACTOR, MIN_FACTOR, 0, +-1, t_bound), zeros of both signs, +-inf, NaN of both signs, subnormals and 1e6 random
 * operands each: (i) "error_norm < 1"; (ii) the step factor against SciPy's min / max written as compares, NaN power
 * included; (iii) "t - t_bound >= 0" on committed steps; (iv) the wait word against the three bools it replaces;
 * (v) the wave-uniform "somebody may be near a boundary" test of Ctx::events, restated: it must hold wherever the per-lane
 * test does.  Exit status 0 and "ok" when everything agrees. */
#define PGR_CR_HOST
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../pygenray_amd/csrc/pgr_crmath.h"

static uint64_t bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static double from_bits(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
/* any bit pattern as an operand -- a NaN made quiet: the kernel's operands are results of arithmetic, never signalling NaNs
   (and fmin on a signalling NaN is the one place where C libraries and the device's canonicalised v_min_f64 may differ) */
static double any_double(uint64_t u) { double d = from_bits(u); return d != d ? from_bits(u | 0x0008000000000000ULL) : d; }
static uint64_t rng_state = 0x2545f4914f6cdd1dULL;
static uint64_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double urand(void) { return (double)(rnd() >> 11) * 0x1p-53; }

#define MIN_FACTOR 0.2
#define MAX_FACTOR 10.0
#define SAFETY 0.9
#define RUNNING (-1)

static long checked = 0;

/* (i) accepted = error_norm < 1 */
static int check_lt(double a, double b, double above)
{
    checked++;
    const int m = pgr_mask_lt_const(a, b, above), want = (a < b) ? -1 : 0;
    if (m != want) { printf("mask_lt_const(%a [%016llx], %a, %a) = %d, a < b is %d\n", a, (unsigned long long)bits(a), b, above, m, want); return 1; }
    return 0;
}

/* (ii) the factor, as rk.py:148-165 was written with compares before */
static double factor_compare_form(int accepted, int rejected_before, double pw)
{
    double fac_acc = (pw < MAX_FACTOR) ? pw : MAX_FACTOR;
    fac_acc = (rejected_before && !(fac_acc < 1)) ? 1.0 : fac_acc;
    const double fac_rej = (pw > MIN_FACTOR) ? pw : MIN_FACTOR;
    return accepted ? fac_acc : fac_rej;
}
static int check_factor(double pw)
{
    int bad = 0;
    for (int acc = 0; acc < 2; acc++)
        for (int rej = 0; rej < 2; rej++) {
            checked++;
            const double want = factor_compare_form(acc, rej, pw);
            const double got = pgr_step_factor(acc ? -1 : 0, pw, pgr_factor_limit(rej ? -1 : 0, MAX_FACTOR), MIN_FACTOR);
            if (bits(want) != bits(got)) { printf("factor(acc %d, rej %d, pw %a): compare form %a, masked form %a\n", acc, rej, pw, want, got); bad++; }
        }
    return bad;
}

/* (iii) status at t >= t_bound: t <= t_bound on a committed step */
static int check_reached(double t, double t_bound)
{
    if (!(t <= t_bound)) return 0;                                       /* (the attempt clamps t_new) */
    if (t == 0.0 && t_bound == 0.0 && signbit(t) && !signbit(t_bound)) return 0;   /* (t = -0 against +0: see pgr_mask_reached) */
    checked++;
    const double d = t - t_bound;
    const int m = pgr_mask_reached(d), want = (d >= 0) ? -1 : 0;
    if (m != want) { printf("mask_reached(%a - %a) = %d, >= 0 is %d\n", t, t_bound, m, want); return 1; }
    /* the kernel's use: status &= ~mask, PGR_RAY_OK = 0 */
    for (int status = -1; status <= 8; status++)
        if ((status & ~m) != ((d >= 0) ? 0 : status)) { printf("status %d & ~mask_reached(%a)\n", status, d); return 1; }
    return 0;
}

/* (v) Ctx::events: near_bottom | near_vertical implies the wave-uniform pre-test */
static int check_near(double pc, double z, double zmin, double k_vert)
{
    checked++;
    const int above = z < zmin;
    const int near_bottom = (pc > 0) & (pc <= 1.0) & !above;
    const int near_vertical = (fabs(pc) > k_vert) & (fabs(pc) <= 1.0);
    const int maybe = !(fabs(pc) <= k_vert) | !(z < zmin);
    if ((near_bottom | near_vertical) && !maybe) { printf("near (pc %a, z %a, zmin %a) without the uniform test\n", pc, z, zmin); return 1; }
    return 0;
}

int main(void)
{
    int bad = 0;
    const double nan_p = from_bits(0x7ff8000000000000ULL), nan_n = from_bits(0xfff8000000000000ULL),
                 nan_p2 = from_bits(0x7ff8000000000001ULL), nan_n2 = from_bits(0xfffc00000000beefULL);
    const double k_vert = 1.0 - 2e-10;
    const double thresholds[] = {1.0, MAX_FACTOR, MIN_FACTOR, 0.0, -1.0, 2.0, k_vert, 1000e3, 100e3};
    const int nt = (int)(sizeof thresholds / sizeof thresholds[0]);
    double ops[256];
    int no = 0;
    for (int i = 0; i < nt; i++) {
        double lo = thresholds[i], hi = thresholds[i];
        ops[no++] = thresholds[i];
        for (int q = 0; q < 3; q++) { lo = nextafter(lo, -INFINITY); hi = nextafter(hi, INFINITY); ops[no++] = lo; ops[no++] = hi; }
    }
    const double more[] = {0.0, -0.0, INFINITY, -INFINITY, nan_p, nan_n, nan_p2, nan_n2, 4.9406564584124654e-324, -4.9406564584124654e-324,
                           2.2250738585072009e-308, -2.2250738585072009e-308, 2.2250738585072014e-308, 0x1.fffffffffffffp+1023,
                           -0x1.fffffffffffffp+1023, 0.5, 1.5, 1e-7, 1e4, 1e-300, 1e300};
    for (int i = 0; i < (int)(sizeof more / sizeof more[0]); i++) ops[no++] = more[i];

    /* (i) */
    for (int i = 0; i < no; i++) {
        bad += check_lt(ops[i], 1.0, 2.0);
        bad += check_lt(ops[i], MAX_FACTOR, 20.0);
        bad += check_lt(ops[i], MIN_FACTOR, 1.0);
        bad += check_lt(ops[i], -1.0, 0.0);
    }
    for (int k = 0; k < 1000000; k++) {
        const double a = (k & 1) ? any_double(rnd()) : ldexp(urand() * 2.0, (int)(rnd() % 40) - 30);   /* any bit pattern / around 1 */
        bad += check_lt(a, 1.0, 2.0);
    }
    /* (ii) */
    for (int i = 0; i < no; i++) { bad += check_factor(ops[i]); bad += check_factor(SAFETY * ops[i]); }
    for (int k = 0; k < 1000000; k++)
        bad += check_factor((k & 1) ? any_double(rnd()) : SAFETY * ldexp(1.0 + urand(), (int)(rnd() % 12) - 6));
    /* (iii) */
    const double bounds[] = {1000e3, 100e3, 1.0, 0.0, -0.0, -5.0, 4.9406564584124654e-324, 0x1.fffffffffffffp+1023, 12345.678};
    for (int b = 0; b < (int)(sizeof bounds / sizeof bounds[0]); b++) {
        double t = bounds[b];
        for (int q = 0; q < 6; q++) { bad += check_reached(t, bounds[b]); t = nextafter(t, -INFINITY); }
        for (int i = 0; i < no; i++) bad += check_reached(ops[i], bounds[b]);
        /* the last step landing exactly on t_bound: t + h rounds onto it */
        for (int k = 0; k < 1000; k++) {
            const double t0 = bounds[b] - fabs(bounds[b]) * urand() - urand(), h = bounds[b] - t0;
            double tn = t0 + h;
            if (tn - bounds[b] > 0) tn = bounds[b];
            bad += check_reached(tn, bounds[b]);
        }
    }
    for (int k = 0; k < 1000000; k++) {
        const double tb = ldexp(urand() - 0.5, (int)(rnd() % 44) - 2);
        double t = tb;
        switch (rnd() % 4) {
        case 0: break;
        case 1: t = nextafter(tb, -INFINITY); break;
        case 2: t = tb - fabs(tb) * urand(); break;
        default: t = tb - ldexp(urand(), (int)(rnd() % 80) - 60); break;
        }
        bad += check_reached(t, tb);
    }
    /* (iv) the wait word against (status == RUNNING && (parked || need_init)), and the head's "this lane steps" */
    for (int status = -1; status <= 8; status++)
        for (int parked = 0; parked < 2; parked++)
            for (int need_init = 0; need_init < 2; need_init++) {
                checked++;
                const int wait = (parked ? PGR_WAIT_PARKED : 0) | (need_init ? PGR_WAIT_INIT : 0);
                const int pend = status == RUNNING && (parked || need_init), steps = status == RUNNING && !parked && !need_init;
                if ((pgr_lane_pending(status, wait) != 0) != pend) { printf("lane_pending(%d, %d)\n", status, wait); bad++; }
                if ((((status ^ RUNNING) | wait) == 0) != steps) { printf("steps(%d, %d)\n", status, wait); bad++; }
                if ((status < 0) != (status == RUNNING)) bad++;
            }
    /* (v) */
    const double zmins[] = {5000.0, -INFINITY, 0.0, 1234.5};
    for (int i = 0; i < no; i++)
        for (int j = 0; j < no; j++)
            for (int q = 0; q < 4; q++) bad += check_near(ops[i], ops[j], zmins[q], k_vert);
    for (int k = 0; k < 1000000; k++) {
        const double pc = (k & 1) ? any_double(rnd()) : (urand() * 2.2 - 1.1);
        const double z = (k & 2) ? any_double(rnd()) : urand() * 6000.0 - 100.0;
        bad += check_near(pc, z, zmins[k & 3], k_vert);
    }
    /* heap use under the sanitizer: the masks over an array, in place */
    const int N = 4096;
    double *v = (double *)malloc(N * sizeof *v);
    int *m = (int *)malloc(N * sizeof *m);
    if (!v || !m) return 2;
    for (int i = 0; i < N; i++) v[i] = urand() * 2.0;
    for (int i = 0; i < N; i++) m[i] = pgr_mask_lt_const(v[i], 1.0, 2.0);
    for (int i = 0; i < N; i++)
        if (m[i] != ((v[i] < 1.0) ? -1 : 0)) bad++;
    free(v);
    free(m);
    printf("%s: %ld predicates checked, %d disagreements\n", bad ? "FAILED" : "ok", checked, bad);
    return bad ? 1 : 0;
}
