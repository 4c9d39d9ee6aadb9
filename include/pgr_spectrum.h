/* pgr_spectrum.h -- the part of the C ABI of libpgr_hip.so that gives the transfer function of a fan's ray-tube arrivals over
 * a band of frequencies.  Included by pgr.h (inside its extern "C" block, after the types it declares); not meant to be
 * included on its own. */
#ifndef PGR_SPECTRUM_H_ABI
#define PGR_SPECTRUM_H_ABI

/* ---- Transfer function over a frequency band ----
 *
 * Groups and arrivals are pgr_signal_device's: group g = j * n + c for receiver j and requested column slot c, arrival a of
 * group g in [offsets[g], offsets[g + 1]), in increasing tube order, with T_a (its travel time), I_a (its intensity) and q_a
 * (int32, its phase index in quarter cycles; < 0: the arrival adds nothing; q NULL: all zero), and L_a, its path length in
 * metres (L NULL: none).  With the frequencies freq[n_freq] in Hz (finite, >= 0), the absorption alpha[n_freq] in dB per
 * METRE (finite, >= 0; NULL: none; given exactly when L is) and a reduction time tred[g] per group, for every group g and
 * frequency index k
 *   re = im = 0.0;  for a = offsets[g] ... offsets[g + 1] - 1 in order:
 *       if q_a < 0: continue
 *       tau = T_a - tred[g]
 *       amp = sqrt(I_a);  y = freq[k] * tau;  y = y - rint(y);  ph = y - 0.25 * (q_a & 3);  ph = ph - rint(ph)
 *       (cv, sv) = cos, sin of 2 pi ph
 *       without alpha:  re = re + amp * cv;          im = im + amp * sv
 *       with alpha:     yw = -((alpha[k] * L_a) * K20);  W = yw != yw ? NaN : (yw < -700.0 ? 0.0 : exp(yw))
 *                       re = re + (amp * cv) * W;    im = im + (amp * sv) * W
 *   re[g * n_freq + k] = re,  im[g * n_freq + k] = im
 * H = re + i im = exp(-i 2 pi f_k tred[g]) sum_a amp_a W_a(f_k) exp(i (2 pi f_k T_a - (pi / 2) q_a)) is the channel's transfer
 * function at f_k, in pgr_fan_pressure_w's sign convention; W = 10^(-alpha L / 20), K20 the double nearest ln(10) / 20.
 * cos / sin and exp are the library's own fixed sequences, the square root correctly rounded, nothing contracted (reference
 * build).  No value is filtered except q_a < 0: a NaN T_a or I_a makes that group's entries NaN.  With tred[g] == 0.0 and no
 * alpha every entry of group g is pgr_fan_pressure_w's value at (j, column) for freq[k], bit for bit in the reference build.
 * freq and alpha are HOST pointers; every other pointer is a DEVICE pointer: offsets int64 [n_groups + 1], T / I / L float64
 * and q int32 [offsets[n_groups]], tred float64 [n_groups], re / im float64 [n_groups][n_freq].  Every output entry is
 * written; an empty group gets zeros.  One lane forms each entry's sums in arrival order: no atomics, repeated calls are
 * bit-equal.  The arguments (null required pointers, L without alpha or alpha without L, n_groups < 1 or beyond INT32_MAX,
 * n_freq < 1 or beyond 65535 * 256, a non-finite or negative freq[k] or alpha[k]) are checked before any device work: a
 * failed check writes nothing.  Enqueued on `stream`, no synchronisation. */
int pgr_spectrum_device(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                        const int32_t* q, const double* L, const double* tred, const double* freq, const double* alpha,
                        int32_t n_freq, double* re, double* im, void* stream);

#endif /* PGR_SPECTRUM_H_ABI */
