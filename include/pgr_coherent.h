/* pgr_coherent.h -- the part of the C ABI of libpgr_hip.so that gives the phase of a fan's ray tubes and their coherent sum.
 * Included by pgr.h (inside its extern "C" block, after the types it declares); not meant to be included on its own. */
#ifndef PGR_COHERENT_H
#define PGR_COHERENT_H

/* ---- Caustic index and coherent ray-tube pressure ----
 *
 * The caustic index.  Tube k is the surviving rays k, k + 1 in launch order; d = the depth at save column s; nb, ns (DEVICE
 * int32 [S][M], as pgr_fan_boundary_loss writes them; NULL: all zero) the rays' per-sample bounce counts.
 *   valid(s): d_k(s), d_k+1(s) not NaN, d_k+1(s) != d_k(s), nb_k(s) == nb_k+1(s), ns_k(s) == ns_k+1(s)
 *   u(s)    = sign(d_k+1(s) - d_k(s)) * (-1)^(nb_k(s) + ns_k(s))      (the tube's width with the mirror flips undone)
 *   sig = 0, n = 0;  for s = 0 ... S - 1 in order: if valid(s) { if sig != 0 and u(s) != sig: n += 1;  sig = u(s) }
 *   kappa[s * M + k] = n  for k = 0 ... M - 2;   kappa[s * M + M - 1] = 0.
 * A tube whose two rays have bounced a different number of times is folded over the boundary: skipped, it carries its last
 * sign, as a NaN sample does.  kappa (DEVICE int32 [S][M]): every entry is written.  One lane owns each tube: no atomics,
 * repeated calls are equal.  Needs M >= 2; checked before any device work.  Enqueued on `stream`, no synchronisation.
 * pgr_fan_caustic_index: a device-resident fan with trajectories (either layout; dropped rays skipped in place; waits for the
 *   fan's kernel).
 * pgr_caustic_index_device: caller rows z (DEVICE) [n_samples][n_rays], stored sign convention, every ray kept.
 *
 * The coherent tube sum.  The arguments of pgr_fan_intensity_w / pgr_intensity_device_w (weights NULL: none), the travel times
 * (the fan's own; T [n_samples][n_rays] for the _device entry), a frequency in Hz (finite, >= 0) and q (DEVICE int32 [S][M],
 * entry [s * M + k] for tube k; NULL: all zero): the tube's phase index in quarter cycles, < 0 for a tube that adds nothing.
 * The tubes counted at receiver j and column s are exactly those pgr_fan_intensity adds there -- the same validity test and
 * the same [lo, hi) -- that also have q >= 0; for each, in increasing k from 0.0,
 *   w = (D_j - d_k) / (d_k+1 - d_k),  T = T_k + w (T_k+1 - T_k)        (pgr_fan_arrivals' bits)
 *   a = sqrt(I_k)                                                      (I_k: the term of pgr_fan_intensity_w, the same bits)
 *   y = f T;  y = y - rint(y);  t = y - 0.25 (q & 3);  t = t - rint(t)
 *   re += a cos(2 pi t),  im += a sin(2 pi t)                          (p = sum of a exp(i (2 pi f T - (pi / 2) q)))
 * with the library's own cos / sin of 2 pi t on [-0.5, 0.5] (a fixed sequence of compares and + - x, absolute error at most
 * 2^-51); division and square root correctly rounded, nothing contracted (reference build).  re, im (DEVICE float64
 * [n_depths][S], every entry written): NaN in the column r_s == 0, 0.0 where no tube reaches.  One lane forms each
 * receiver's sums in tube order: no atomics, repeated calls are bit-equal. */
int pgr_fan_caustic_index(pgr_fan* fan, const int32_t* nb, const int32_t* ns, int32_t* kappa, void* stream);
int pgr_caustic_index_device(int device, const double* z, int64_t n_rays, int32_t n_samples, const int32_t* nb,
                             const int32_t* ns, int32_t* kappa, void* stream);
int pgr_fan_pressure_w(pgr_fan* fan, const double* p0, const double* weights, const int32_t* q, double frequency,
                       const double* depths, int64_t n_depths, double* re, double* im, void* stream);
int pgr_pressure_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                          int32_t n_samples, const double* x, const double* p0, const double* weights, const int32_t* q,
                          double frequency, const double* depths, int64_t n_depths, double* re, double* im, void* stream);

#endif /* PGR_COHERENT_H */
