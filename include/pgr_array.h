/* pgr_array.h -- the part of the C ABI of libpgr_hip.so that gives the time-angle response of a vertical line array:
 * delay-and-sum beamforming over the elements' arrival lists.  Included by pgr.h (inside its extern "C" block, after
 * pgr_beam_arrivals.h); not meant to be included on its own. */
#ifndef PGR_ARRAY_H_ABI
#define PGR_ARRAY_H_ABI

/* ---- Vertical-array beamforming ----
 *
 * The arrival lists are pgr_signal_device's (pgr_signal.h): group g = j * n_cols + c for element j of n_elements and column
 * slot c, arrival a of group g in [offsets[g], offsets[g + 1]), with T_a, I_a, q_a (q NULL: all zero) and, when phi is not
 * NULL, its lag in cycles phi_a (pgr_reflection.h).  With a delay in seconds per group and look, delay[g * n_looks + b], a
 * weight per group, weight[g], a start time per column slot, tstart[c], and the pulse of pgr_signal_device (frequency f,
 * rs = inv_sigma, dt, n_times), for every column slot c, look b and sample n
 *   t_n = tstart[c] + (double)n * dt
 *   re = im = 0.0
 *   for j = 0 ... n_elements - 1:  g = j * n_cols + c;  dl = delay[g * n_looks + b];  w = weight[g]
 *     for a = offsets[g] ... offsets[g + 1] - 1 in order:
 *       if q_a < 0: continue
 *       Ts = T_a - dl
 *       x = (t_n - Ts) * rs;  v = x * x;  if !(v <= 64.0): continue           (a NaN T_a or delay adds nothing)
 *       amp = sqrt(I_a);  amp = amp * w
 *       y = f * Ts;  y = y - rint(y);  ph = y - 0.25 * (q_a & 3);  ph = ph - rint(ph)
 *       if phi:  r = phi_a - rint(phi_a);  ph = ph - r;  ph = ph - rint(ph)
 *       (cv, sv) = cos, sin of 2 pi ph;   E = exp(-0.5 * v)
 *       re = re + (amp * cv) * E;    im = im + (amp * sv) * E
 *   re[(c * n_looks + b) * n_times + n] = re,  im[...] = im
 * This is baseband delay-and-sum in pgr_signal_device's convention (the analytic signal is u(t) exp(-i 2 pi f t)):
 *   y(t) = sum_j w_j exp(-i 2 pi f dl_j) u_j(t + dl_j),
 * the shift T_a - dl giving both the phase factor and the delayed envelope.  cos / sin, exp and the square root are
 * pgr_signal_device's, nothing contracted (reference build).  With n_elements = 1, every delay 0.0 and every weight 1.0 the
 * result is pgr_signal_device's (with phi pgr_signal_device_phi's) bit for bit; at rs = 0 it is the CW conventional beamformer.
 * All pointers are DEVICE pointers: offsets int64 [n_elements * n_cols + 1], T / I / phi float64 and q int32
 * [offsets[n_elements * n_cols]], delay float64 [n_elements * n_cols][n_looks], weight float64 [n_elements * n_cols], tstart
 * float64 [n_cols], re / im float64 [n_cols][n_looks][n_times].  Every output entry is written.  One lane forms each sample's
 * sums in element and arrival order: no atomics, repeated calls are bit-equal.  The arguments are checked before any device
 * work -- pgr_signal_device's checks (with n_groups = n_elements * n_cols), a null delay or weight, n_elements, n_cols or
 * n_looks < 1, n_cols * n_looks beyond INT32_MAX -- and a failed check writes nothing.  Enqueued on `stream`, no
 * synchronisation. */
int pgr_array_response_device(int device, const int64_t* offsets, int64_t n_elements, int64_t n_cols, const double* T,
                              const double* I, const int32_t* q, const double* phi, const double* delay, const double* weight,
                              const double* tstart, double frequency, double inv_sigma, double dt, int32_t n_times,
                              int64_t n_looks, double* re, double* im, void* stream);

#endif /* PGR_ARRAY_H_ABI */
