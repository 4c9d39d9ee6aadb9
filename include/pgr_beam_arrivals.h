/* pgr_beam_arrivals.h -- the part of the C ABI of libpgr_hip.so that lists the terms of the coherent Gaussian-beam sum as
 * arrivals, per receiver and requested save column.  Included by pgr.h (inside its extern "C" block, after
 * pgr_beam_coherent.h); not meant to be included on its own. */
#ifndef PGR_BEAM_ARRIVALS_H_ABI
#define PGR_BEAM_ARRIVALS_H_ABI

/* ---- Gaussian-beam arrivals ----
 *
 * Every term pgr_fan_beam_pressure_w / pgr_beam_pressure_device_w adds at a receiver is one arrival: its delay, its amplitude
 * and its phase index do not depend on the frequency.  The fan, p0, weights, q, bottom, depths, min_width and curvature are
 * those entries' (pgr_beam_coherent.h, whose notation this uses); cols[n_cols] is a HOST list of save columns as
 * pgr_fan_arrivals_w takes it (any order, duplicates allowed, 1 .. 65535 of them): slot c is column s = cols[c].
 * For receiver j and slot c, nothing when r_s == 0 (the source's own column); else for k = 0 .. M - 2 in order, where tube k
 * adds its terms (g finite at both ends, weights included, and q[s][k] >= 0; q NULL: 0), for the centres m_k, -m_k,
 * 2 b_s - m_k in that order (image 0, 1, 2; dq = 0, 2, 0), with e0 = d_j - centre: the term is kept when
 * |e0| <= sigma_k GB_REACH and v = (e0 / sigma_k)^2 <= 16 -- the same operations as the pressure entries' -- and is then one
 * arrival
 *   tube      = k                                   int32
 *   image     = 0 the beam, 1 its surface image, 2 its bottom image      int32
 *   time      = T_m + (p_m e + hk (e e))            e: the receiver mirrored with the image, in the beam's own space
 *   amplitude = A'_k gexp(-0.5 v)
 *   qa        = (q_k + dq) & 3                      int32
 * the set, the order and every value exactly what the pressure entries form before their trigonometry (reference build): the
 * arrivals of a group, summed by pgr_spectrum_device with I = amplitude * amplitude at a frequency f, give the pressure entries'
 * re / im at f bit for bit wherever no amplitude's square underflows and no time is NaN.
 *   counts [n_depths][n_cols] int64 (DEVICE): the arrivals of group g = j * n_cols + c, every entry written;
 *   offsets [n_depths * n_cols] int64 (DEVICE): the caller's exclusive scan of the counts; group g's arrivals are written, in
 *   the order above, from offsets[g] into tube / image / time / amplitude / qa (DEVICE, n_arrivals each); writes at or past
 *   n_arrivals are dropped.
 * One lane finds and writes each receiver's arrivals in order: no atomics, repeated calls are bit-equal.
 * Refused before any device work, with nothing written: a null argument (weights and q may be NULL), a min_width that is not
 * finite and > 0, fewer than two rays, n_cols outside 1 .. 65535, a column outside 0 .. n_samples - 1, n_arrivals < 1 (skip
 * the call when there are none).  The layouts, the waiting for the fan's kernel and the stream are the pressure entries'. */
int pgr_fan_beam_arrival_counts_w(pgr_fan* fan, const double* p0, const double* weights, const int32_t* q,
                                  const double* bottom, const double* depths, int64_t n_depths, double min_width,
                                  const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream);
int pgr_fan_beam_arrivals_w(pgr_fan* fan, const double* p0, const double* weights, const int32_t* q, const double* bottom,
                            const double* depths, int64_t n_depths, double min_width, const int32_t* cols, int32_t n_cols,
                            int32_t curvature, const int64_t* offsets, int64_t n_arrivals, int32_t* tube, int32_t* image,
                            double* time, double* amplitude, int32_t* qa, void* stream);
int pgr_beam_arrival_counts_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                                     int32_t n_samples, const double* x, const double* p0, const double* weights,
                                     const int32_t* q, const double* bottom, const double* depths, int64_t n_depths,
                                     double min_width, const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream);
int pgr_beam_arrivals_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                               int32_t n_samples, const double* x, const double* p0, const double* weights, const int32_t* q,
                               const double* bottom, const double* depths, int64_t n_depths, double min_width,
                               const int32_t* cols, int32_t n_cols, int32_t curvature, const int64_t* offsets,
                               int64_t n_arrivals, int32_t* tube, int32_t* image, double* time, double* amplitude, int32_t* qa,
                               void* stream);

#endif /* PGR_BEAM_ARRIVALS_H_ABI */
