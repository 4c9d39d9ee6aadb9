/* pgr_beam_coherent.h -- the part of the C ABI of libpgr_hip.so that gives the coherent sum of a fan's geometric Gaussian
 * beams, with the wavefront curvature across each tube.  Included by pgr.h (inside its extern "C" block, after
 * pgr_reflection.h); not meant to be included on its own. */
#ifndef PGR_BEAM_COHERENT_H
#define PGR_BEAM_COHERENT_H

/* ---- Coherent Gaussian-beam pressure ----
 *
 * The arguments of pgr_fan_beam_intensity_w / pgr_beam_intensity_device_w (weights NULL: none; bottom DEVICE float64 [S], the
 * bottom depth at each save range; min_width finite and > 0), the travel times (the fan's own; T [n_samples][n_rays] for the
 * _device entry), a frequency in Hz (finite, >= 0), q (DEVICE int32 [S][M], entry [s * M + k] for tube k; NULL: all zero): the
 * tube's phase index in quarter cycles as pgr_fan_pressure_w takes it, < 0 for a tube that adds nothing, and `curvature`
 * (0: every hk below is 0.0, the plain geometric beam).
 * Per save column s and tube k (surviving rays k, k + 1): d the depths, T the travel times, p the slowness along increasing
 * depth (dT/dd at a fixed range: the stored p with the sign the stored z takes to become a depth -- an exact operation), g
 * weighted as in the _w entries.  E_k, D_k = |d_k+1 - d_k|, sigma_k and m_k are pgr_fan_beam_intensity's, bit for bit, and
 *   T_m = 0.5 (T_k + T_k+1),   p_m = 0.5 (p_k + p_k+1)
 *   hk  = curvature && D_k > 0 ? 0.5 * ((p_k+1 - p_k) / (d_k+1 - d_k)) : 0.0
 *   A'_k = sqrt(E_k * D_k) / (sigma_k SQRT_2PI)                        (Gaussians sigma wide and D apart, in phase, sum to
 *                                                                       sqrt(E / D), the tube's amplitude; D_k = 0 adds +0)
 * A tube adds its terms when pgr_fan_beam_intensity's does (g finite at both ends) and q >= 0.  Receiver j takes the centres in
 * pgr_fan_beam_intensity's order, each with that entry's own v = ((d_j - centre) / sigma_k)^2 and its v <= 16 test:
 *   centre         e, the receiver in the beam's own space     quarter cycles dq
 *   m_k            d_j - m_k                                   0
 *   -m_k           (-d_j) - m_k                                2     (a pressure-release surface)
 *   2 b_s - m_k    (2 b_s - d_j) - m_k                         0     (a rigid bottom)
 *   a   = A'_k gexp(-0.5 v)
 *   tau = T_m + (p_m e + hk (e e))
 *   y = f tau;  y = y - rint(y);  t = y - 0.25 ((q + dq) & 3);  t = t - rint(t)
 *   re += a cos(2 pi t),  im += a sin(2 pi t)
 * from 0.0 in increasing k and, per tube, in centre order, with the library's exp of the beam intensity and its cos / sin of
 * the coherent tube sum; division and square root correctly rounded, nothing contracted (reference build).  re, im (DEVICE
 * float64 [n_depths][S], every entry written): NaN in the column r_s == 0, 0.0 where no beam reaches.  One lane forms each
 * receiver's two sums in that order: no atomics, repeated calls are bit-equal.
 * hk is half the wavefront curvature Delta p / Delta d across the tube.  It grows without bound at a caustic, where D -> 0,
 * while A' -> 0 there: the sum stays bounded by the sum of the A' of the beams that reach the receiver.
 * A min_width that is not finite and > 0, a frequency that is not finite and >= 0 and fewer than two rays are refused before
 * any device work, with nothing written; every other check, the layouts (either trajectory layout, dropped rays skipped in
 * place), the waiting for the fan's kernel and the stream are pgr_fan_beam_intensity_w's / pgr_beam_intensity_device_w's. */
int pgr_fan_beam_pressure_w(pgr_fan* fan, const double* p0, const double* weights, const int32_t* q, double frequency,
                            const double* bottom, const double* depths, int64_t n_depths, double min_width,
                            int32_t curvature, double* re, double* im, void* stream);
int pgr_beam_pressure_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                               int32_t n_samples, const double* x, const double* p0, const double* weights,
                               const int32_t* q, double frequency, const double* bottom, const double* depths,
                               int64_t n_depths, double min_width, int32_t curvature, double* re, double* im, void* stream);

#endif /* PGR_BEAM_COHERENT_H */
