/* pgr_band.h -- the part of the C ABI of libpgr_hip.so that gives the power of a fan's arrivals summed over a band of
 * frequencies, the quantity behind band-averaged transmission loss.  Included by pgr.h (inside its extern "C" block, after
 * pgr_array.h); not meant to be included on its own. */
#ifndef PGR_BAND_H_ABI
#define PGR_BAND_H_ABI

/* ---- Band-averaged power ----
 *
 * Groups, arrivals, frequencies and absorption are pgr_spectrum_device's (pgr_spectrum.h): arrival a of group g in
 * [offsets[g], offsets[g + 1]) with T_a, I_a, q_a (q NULL: all zero) and L_a (L NULL: none), freq[n_freq] in Hz and
 * alpha[n_freq] in dB per METRE (given exactly when L is); phi, when not NULL, holds every arrival's lag in cycles
 * (pgr_reflection.h).  There is no reduction time: tau = T_a.  With the band weights wf[n_freq] (finite, >= 0), for every group g
 *   for k = 0 ... n_freq - 1:
 *       (re_k, im_k) = pgr_spectrum_device's sums for (g, k) with tred[g] = 0.0 -- with phi pgr_spectrum_device_phi's, i.e. behind
 *                      ph = ph - rint(ph) also  r = phi_a - rint(phi_a);  ph = ph - r;  ph = ph - rint(ph)  -- the same
 *                      operations in the same order
 *       P_k = re_k * re_k + im_k * im_k                                  (two products, one add)
 *   s_l = 0.0 for l = 0 ... 63
 *   for k = l, l + 64, l + 128, ... < n_freq in increasing k:  s_l = s_l + wf[k] * P_k
 *   for d = 32, 16, 8, 4, 2, 1:  s_l = s_l + s_(l xor d)                  (every l at once; the 64 values end equal)
 *   out[g] = s_0
 * which is sum_k wf[k] |H(f_k)|^2 in a fixed order, H the transfer function of pgr_spectrum_device -- never stored.  Nothing is
 * contracted (reference build).  An empty group gives +0.0; q_a < 0 adds nothing; a NaN T_a, I_a or lag makes out[g] NaN.  With
 * n_freq = 1 and wf[0] = 1.0, out[g] is re * re + im * im of pgr_fan_pressure_w's value, bit for bit in the reference build.
 * freq, alpha and wf are HOST pointers; every other pointer is a DEVICE pointer: offsets int64 [n_groups + 1], T / I / phi / L
 * float64 and q int32 [offsets[n_groups]], out float64 [n_groups].  Every out[g] is written.  One wave forms a group's value in
 * the order above: no atomics, repeated calls are bit-equal.  The arguments are checked before any device work -- everything
 * pgr_spectrum_device refuses, a null wf or out, a non-finite or negative wf[k] -- and a failed check writes nothing.  Enqueued
 * on `stream`, no synchronisation. */
int pgr_band_power_device(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                          const int32_t* q, const double* phi, const double* L, const double* freq, const double* alpha,
                          const double* wf, int32_t n_freq, double* out, void* stream);

#endif /* PGR_BAND_H_ABI */
