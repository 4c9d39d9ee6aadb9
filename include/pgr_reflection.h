/* pgr_reflection.h -- the part of the C ABI of libpgr_hip.so that gives the coherent sums with a real phase per arrival: the
 * bottom's complex reflection coefficient.  Included by pgr.h (inside its extern "C" block, after pgr_spectrum.h); not meant
 * to be included on its own. */
#ifndef PGR_REFLECTION_H_ABI
#define PGR_REFLECTION_H_ABI

/* ---- The coherent sums with an accumulated lag per arrival ----
 *
 * Each entry is its sibling's prototype (pgr_fan_pressure_w, pgr_pressure_device_w, pgr_signal_device, pgr_spectrum_device) with
 * one more pointer, phi, directly after q: a lag in CYCLES (any finite value; whole cycles change nothing) that the arrival's
 * phase is turned back by, on top of its quarter cycles q.
 *   tube sums     phi: DEVICE float64 [S][M], entry [s * M + m] the lag ray m has collected up to save column s (what
 *                 pgr_fan_boundary_loss writes when the bottom's table holds lags instead of dB).  The arrival of tube k gets
 *                     d = Phi_k+1 - Phi_k;  d = w * d;  phi_a = Phi_k + d       (w: the arrival's own bits; three roundings)
 *   arrival sums  phi: DEVICE float64 [offsets[n_groups]], phi_a of every arrival.
 * The term is the sibling's own operations in its order, with
 *   r = phi_a - rint(phi_a)
 *   t = ... the sibling's t (or ph) after its own  t = t - rint(t) ...
 *   t = t - r;  t = t - rint(t)                                            then cos, sin of 2 pi t as before
 * so the arrival adds  a exp(i (2 pi f T - (pi / 2) q - 2 pi phi_a)).  Nothing is contracted in the reference build.  With phi
 * all zero, or any whole numbers of cycles, r = 0 and both added operations leave t's bits alone (|t| <= 0.5, ties to even):
 * every entry then returns its sibling's result bit for bit (reference build).  A NaN phi makes the sums it enters NaN by IEEE
 * rules (in pgr_signal_device_phi: the samples within 8 sigma of that arrival).  Tubes / arrivals with q < 0 still add nothing
 * and their phi is not read into the sums.
 * phi NULL is refused: the caller uses the sibling.  Every other check, refusal, layout and guarantee (every output entry
 * written, no atomics, repeated calls bit-equal, a failed check writes nothing, enqueued on `stream` without synchronisation)
 * is the sibling's. */
int pgr_fan_pressure_phi(pgr_fan* fan, const double* p0, const double* weights, const int32_t* q, const double* phi,
                         double frequency, const double* depths, int64_t n_depths, double* re, double* im, void* stream);
int pgr_pressure_device_phi(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                            int32_t n_samples, const double* x, const double* p0, const double* weights, const int32_t* q,
                            const double* phi, double frequency, const double* depths, int64_t n_depths, double* re,
                            double* im, void* stream);
int pgr_signal_device_phi(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                          const int32_t* q, const double* phi, const double* tstart, double frequency, double inv_sigma,
                          double dt, int32_t n_times, double* re, double* im, void* stream);
int pgr_spectrum_device_phi(int device, const int64_t* offsets, int64_t n_groups, const double* T, const double* I,
                            const int32_t* q, const double* phi, const double* L, const double* tred, const double* freq,
                            const double* alpha, int32_t n_freq, double* re, double* im, void* stream);

#endif /* PGR_REFLECTION_H_ABI */
