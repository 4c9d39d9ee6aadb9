/* pgr_signal.h -- the part of the C ABI of libpgr_hip.so that gives the received time series of a Gaussian pulse from a fan's
 * ray-tube arrivals.  Included by pgr.h (inside its extern "C" block, after the types it declares); not meant to be included
 * on its own. */
#ifndef PGR_SIGNAL_H_ABI
#define PGR_SIGNAL_H_ABI

/* ---- Received signal of a Gaussian pulse ----
 *
 * Arrivals come in groups, in pgr_fan_arrivals' order: group g = j * n + c for receiver j and requested column slot c, and
 * arrival a of group g lies in [offsets[g], offsets[g + 1]), in increasing tube order.  Per arrival: T_a (its travel time),
 * I_a (its intensity: the weighted term of the TL sum, as pgr_fan_arrivals_w writes it) and q_a (int32, its phase index in
 * quarter cycles, as pgr_fan_pressure_w takes it per tube; < 0: the arrival adds nothing; q NULL: all zero).  With the centre
 * frequency f = `frequency` in Hz (finite, >= 0), rs = `inv_sigma` = 1 / sigma in 1 / s (finite, >= 0; 0: the CW limit),
 * dt > 0, n_times >= 1 and a start time tstart[g] per group, for every group g and sample n
 *   t_n = tstart[g] + (double)n * dt
 *   re = im = 0.0;  for a = offsets[g] ... offsets[g + 1] - 1 in order:
 *       if q_a < 0: continue
 *       x = (t_n - T_a) * rs;  v = x * x;  if !(v <= 64.0): continue          (a NaN T_a adds nothing)
 *       amp = sqrt(I_a);  y = f * T_a;  y = y - rint(y);  ph = y - 0.25 * (q_a & 3);  ph = ph - rint(ph)
 *       (cv, sv) = cos, sin of 2 pi ph;   E = exp(-0.5 * v)
 *       re = re + (amp * cv) * E;    im = im + (amp * sv) * E
 *   re[g * n_times + n] = re,  im[g * n_times + n] = im
 * u = re + i im is the complex baseband signal of the Gaussian pulse E(tau) = exp(-tau^2 / (2 sigma^2)), cut at 8 sigma
 * (E = e^-32 = 1.3e-14); the analytic passband signal is u(t) exp(-i 2 pi f t), in pgr_fan_pressure_w's sign convention.
 * cos / sin and exp are the library's own fixed sequences (those of pgr_fan_pressure_w and of pgr_fan_beam_intensity; exp is
 * called on [-32, 0]), the square root correctly rounded, nothing contracted (reference build); t_n is not contracted in
 * either build.  At rs = 0 every term has E = exp(-0.0) = 1.0 exactly, so every sample of group g is pgr_fan_pressure_w's
 * value at (j, column), bit for bit in the reference build.
 * All pointers are DEVICE pointers: offsets int64 [n_groups + 1], T / I float64 and q int32 [offsets[n_groups]], tstart
 * float64 [n_groups], re / im float64 [n_groups][n_times].  Every output entry is written; an empty group gets zeros.  One
 * lane forms each sample's sums in arrival order: no atomics, repeated calls are bit-equal.  The arguments (null pointers,
 * n_groups < 1, n_times < 1 or beyond 65535 * 256, a non-finite or negative frequency / inv_sigma, a non-finite or non-positive
 * dt) are checked before any device work: a failed check writes nothing.  Enqueued on `stream`, no synchronisation. */
int pgr_signal_device(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I, const int32_t* q,
                      const double* tstart, double frequency, double inv_sigma, double dt, int32_t n_times,
                      double* re, double* im, void* stream);

#endif /* PGR_SIGNAL_H_ABI */
