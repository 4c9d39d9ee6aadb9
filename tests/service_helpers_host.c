/* Stand-alone host program over the host twins of the helpers the bounce service's replay uses (pgr_sign_mask,
 * pgr_mask_select: pygenray_amd/csrc/pgr_crmath.h with PGR_CR_HOST) -- TEST INFRASTRUCTURE ONLY, CPU build:
 *   gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=gnu99 -ffp-contract=off \
 *       tests/service_helpers_host.c -lm -o service_helpers_host && ./service_helpers_host
 * (i) the mask select against the compare select on every ordering of neighbouring doubles, zeros of both signs, subnormal
 * differences and the largest finite values; (ii) the replayed halvings in the masked form (as the kernel runs them) against
 * the compare form (as they were written before) on random brackets and bands: the same ends and the same last decision after
 * every halving, bit for bit; (iii) brentq's last iterations likewise.  Exit status 0 and "ok" when everything agrees. */
#define PGR_CR_HOST
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../pygenray_amd/csrc/pgr_crmath.h"

static uint64_t bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double urand(void) { return (double)(rnd() >> 11) * 0x1p-53; }

static int check_pair(double a, double b)
{
    /* all ones exactly where a < b (zeros of different signs aside: (-0) - (+0) = -0, and the service's operands are never
       zeros -- halvings are taken on steps that do not contain x = 0) */
    if (a == 0.0 && b == 0.0) return 0;
    const int m = pgr_sign_mask(a - b);
    if (m != ((a < b) ? -1 : 0)) { printf("sign_mask(%a - %a) = %d\n", a, b, m); return 1; }
    const double s = pgr_mask_select(m, a, b), w = (a < b) ? a : b;
    if (bits(s) != bits(w)) { printf("mask_select(%d, %a, %a) = %a\n", m, a, b, s); return 1; }
    return 0;
}

int main(void)
{
    int bad = 0;
    const double specials[] = {0.0, -0.0, 4.9406564584124654e-324, -4.9406564584124654e-324, 2.2250738585072014e-308,
                               1.0, -1.0, 1e5, 1e6, 0x1.fffffffffffffp+1023, -0x1.fffffffffffffp+1023, 12345.678, 1e-300};
    const int ns = (int)(sizeof specials / sizeof specials[0]);
    for (int i = 0; i < ns; i++)
        for (int j = 0; j < ns; j++) {
            /* (the two largest finite values of opposite sign overflow in the difference: +-inf keeps the right sign) */
            bad += check_pair(specials[i], specials[j]);
            bad += check_pair(specials[i], nextafter(specials[i], specials[j]));
        }
    for (int k = 0; k < 2000000; k++) {
        const double a = ldexp(urand() - 0.5, (int)(rnd() % 80) - 40);
        double b = a;
        const int steps = (int)(rnd() % 4);
        for (int q = 0; q < steps; q++) b = nextafter(b, (rnd() & 1) ? INFINITY : -INFINITY);
        bad += check_pair(a, b);
        bad += check_pair(b, a);
    }
    /* the halvings: brackets [t, t + h] as the service meets them, bands of zero to a few doubles around a point inside */
    long halvings = 0;
    for (int k = 0; k < 200000 && !bad; k++) {
        const double t = ldexp(1.0 + urand(), (int)(rnd() % 21)), h = t * urand() * 0.9 + 1e-3;
        const double t_new = t + h, xs = t + urand() * (t_new - t);
        double xa = xs, xb = xs;
        for (int q = (int)(rnd() % 3); q > 0; q--) xa = nextafter(xa, -INFINITY);
        for (int q = 1 + (int)(rnd() % 3); q > 0; q--) xb = nextafter(xb, INFINITY);
        if (xa < t) xa = t;
        if (xb > t_new) xb = t_new;
        double plo = t, phi = t_new, mlo = t, mhi = t_new;
        int lastc = 1, lastm = -1;
        const int n = (int)(rnd() % 60);
        for (int it = 0; it < n; it++, halvings++) {
            /* the compare form */
            const double nw = __builtin_fma(phi - plo, 0.5, plo);
            const int ge = (nw >= xb), le = (nw <= xa);
            phi = ge ? nw : phi;
            plo = le ? nw : plo;
            lastc = ge | (lastc & !le);
            /* the masked form */
            const double mw = __builtin_fma(mhi - mlo, 0.5, mlo);
            const int m_lt = pgr_sign_mask(mw - xb), m_gt = pgr_sign_mask(xa - mw);
            mhi = pgr_mask_select(m_lt, mhi, mw);
            mlo = pgr_mask_select(m_gt, mlo, mw);
            lastm = ~m_lt | (lastm & m_gt);
            if (bits(phi) != bits(mhi) || bits(plo) != bits(mlo) || (lastm != 0) != (lastc != 0) || (lastm != 0 && lastm != -1)) {
                printf("halving %d of bracket %a + %a, band [%a, %a]: compare form (%a, %a, %d), masked form (%a, %a, %d)\n",
                       it, t, h, xa, xb, plo, phi, lastc, mlo, mhi, lastm);
                bad++;
                break;
            }
        }
        const double cur = lastc ? phi : plo, other = lastc ? plo : phi;
        if (bits(pgr_mask_select(lastm, mhi, mlo)) != bits(cur) || bits(pgr_mask_select(lastm, mlo, mhi)) != bits(other)) bad++;
    }
    /* brentq's last iterations (phase 2 of the replay): the compare form as scipy/optimize/Zeros/brentq.c runs them against
       the masked form, from a bracket a few tolerances wide around a flip at xb (not fired below it, fired from it on; a band
       of no width: every iterate is decided by position) -- the same iterates, the same root */
    long iterations = 0;
    for (int k = 0; k < 300000 && !bad; k++) {
        const double xtol = 4 * 2.220446049250313e-16, brtol = xtol;
        const double x = ldexp(1.0 + urand(), (int)(rnd() % 21)) * ((rnd() & 1) ? 1.0 : -1.0);
        double lo = x, hi = x;
        for (int q = 1 + (int)(rnd() % 40); q > 0; q--) lo = nextafter(lo, -INFINITY);
        for (int q = (int)(rnd() % 40); q > 0; q--) hi = nextafter(hi, INFINITY);
        const double xb = x, xa = nextafter(x, -INFINITY);
        const int start_hi = (int)(rnd() & 1);
        double cur = start_hi ? hi : lo, xblk = start_hi ? lo : hi, fcv = start_hi ? 1.0 : 0.0;
        double mcur = cur, mblk = xblk;
        int fcm = start_hi ? -1 : 0, done = 0, m_done = 0;
        for (int it = 0; it < 100; it++, iterations++) {
            {   /* compare form */
                const double dlt = (xtol + brtol * fabs(cur)) / 2, sbis = (xblk - cur) / 2;
                done = fabs(sbis) < dlt;
                if (!done) {
                    const double nw = (fabs(sbis) > dlt) ? cur + sbis : cur + (sbis > 0 ? dlt : -dlt);
                    const double fnv = (nw >= xb) ? 1.0 : 0.0;
                    xblk = (fnv != fcv) ? cur : xblk;
                    cur = nw;
                    fcv = fnv;
                }
            }
            {   /* masked form */
                const double dlt = (xtol + brtol * fabs(mcur)) / 2, sbis = (mblk - mcur) / 2, asb = fabs(sbis);
                m_done = pgr_sign_mask(asb - dlt);
                const double nw = mcur + pgr_mask_select(pgr_sign_mask(dlt - asb), sbis, __builtin_copysign(dlt, sbis));
                const int m_ltb = pgr_sign_mask(nw - xb);
                const int m_in = ~m_done & pgr_sign_mask(xa - nw) & m_ltb;
                const int m_go = ~(m_done | m_in);
                if (m_in) { printf("an iterate inside a band of no width: %a in (%a, %a)\n", nw, xa, xb); bad++; break; }
                mblk = pgr_mask_select(m_go & (~m_ltb ^ fcm), mcur, mblk);
                mcur = pgr_mask_select(m_go, nw, mcur);
                fcm = (~m_ltb & m_go) | (fcm & ~m_go);
            }
            if (bits(cur) != bits(mcur) || bits(xblk) != bits(mblk) || (fcv != 0.0) != (fcm != 0) || done != (m_done != 0)) {
                printf("brentq iteration %d around %a: compare form (%a, %a, %g, %d), masked form (%a, %a, %d, %d)\n",
                       it, x, cur, xblk, fcv, done, mcur, mblk, fcm, m_done);
                bad++;
                break;
            }
            if (done) break;
        }
        if (!done) { printf("no convergence around %a\n", x); bad++; }
    }
    /* heap use under the sanitizer: the masks over an array, in place */
    const int N = 4096;
    double *v = (double *)malloc(N * sizeof *v);
    if (!v) return 2;
    for (int i = 0; i < N; i++) v[i] = urand() - 0.5;
    for (int i = 0; i + 1 < N; i++) {
        const double lo = pgr_mask_select(pgr_sign_mask(v[i] - v[i + 1]), v[i], v[i + 1]);
        if (lo != ((v[i] < v[i + 1]) ? v[i] : v[i + 1])) bad++;
    }
    free(v);
    printf("%s: %ld halvings and %ld brentq iterations replayed, %d disagreements\n", bad ? "FAILED" : "ok", halvings, iterations, bad);
    return bad ? 1 : 0;
}
