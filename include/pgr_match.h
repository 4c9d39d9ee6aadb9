/* pgr_match.h -- the part of the C ABI of libpgr_hip.so that gives the Bartlett ambiguity surface of matched-field processing
 * from the arrival lists of one fan per array element.  Included by pgr.h (inside its extern "C" block, after pgr_array.h and
 * before pgr_band.h); not meant to be included on its own. */
#ifndef PGR_MATCH_H_ABI
#define PGR_MATCH_H_ABI

/* ---- Matched-field processing ----
 *
 * n_elements elements j and n_cells cells g: the arrival lists of the n_elements * n_cells groups stand element-major, group
 * e = j * n_cells + g in [offsets[e], offsets[e + 1]).  Arrivals, frequencies and absorption are pgr_spectrum_device's
 * (pgr_spectrum.h): T_a, I_a, q_a (q NULL: all zero) and L_a (L NULL: none), freq[n_freq] in Hz and alpha[n_freq] in dB per
 * METRE (given exactly when L is); phi, when not NULL, holds every arrival's lag in cycles (pgr_reflection.h).  There is no
 * reduction time: tau = T_a.  With the band weights wf[n_freq] (finite, >= 0) and the array's data d_re, d_im
 * [n_elements][n_freq] (finite), for every cell g
 *   for k = 0 ... n_freq - 1:
 *       cr = ci = nn = 0.0
 *       for j = 0 ... n_elements - 1 in increasing j:
 *           (re, im) = pgr_spectrum_device's sums for group (j * n_cells + g, k) with tred = 0.0 -- with phi
 *                      pgr_spectrum_device_phi's -- the same operations in the same order
 *           cr = cr + (re * d_re[j][k] + im * d_im[j][k])                 (two products, one add, one add)
 *           ci = ci + (re * d_im[j][k] - im * d_re[j][k])                 (two products, one subtract, one add)
 *           nn = nn + (re * re + im * im)
 *       A = cr * cr + ci * ci
 *       B_k = A when normalize is 0;  when it is 1:  nn == 0.0 ? 0.0 : A / nn   (IEEE division; a NaN nn gives NaN)
 *   s_l = 0.0 for l = 0 ... 63
 *   for k = l, l + 64, l + 128, ... < n_freq in increasing k:  s_l = s_l + wf[k] * B_k
 *   for d = 32, 16, 8, 4, 2, 1:  s_l = s_l + s_(l xor d)                  (every l at once; the 64 values end equal)
 *   out[g] = s_0
 * which is sum_k wf[k] |sum_j conj(H_j(f_k)) d_j(f_k)|^2, with normalize over sum_j |H_j(f_k)|^2, in a fixed order: the Bartlett
 * processor with the replica H_j(f_k) of element j for a source in cell g, H the transfer function of pgr_spectrum_device --
 * never stored.  Nothing is contracted (reference build).  A cell no element reaches gives +0.0; q_a < 0 adds nothing; a NaN
 * T_a, I_a or lag in one of a cell's lists makes that cell NaN and no other.  freq, alpha, wf, d_re and d_im are HOST
 * pointers; every other pointer is a DEVICE pointer: offsets int64 [n_elements * n_cells + 1], T / I / phi / L float64 and q
 * int32 [offsets[n_elements * n_cells]], out float64 [n_cells].  Every out[g] is written.  One wave forms a cell's value in the
 * order above: no atomics, repeated calls are bit-equal.  The arguments are checked before any device work -- everything
 * pgr_spectrum_device refuses of the n_elements * n_cells groups, n_elements or n_cells below 1, more than INT32_MAX groups, a
 * null wf, d_re, d_im or out, a non-finite or negative wf[k], a non-finite datum, a normalize other than 0 or 1 -- and a failed
 * check writes nothing.  Enqueued on `stream`, no synchronisation. */
int pgr_matched_field_device(int device, const int64_t* offsets, int32_t n_elements, int64_t n_cells, const double* T,
                             const double* I, const int32_t* q, const double* phi, const double* L, const double* freq,
                             const double* alpha, const double* wf, const double* d_re, const double* d_im, int32_t n_freq,
                             int normalize, double* out, void* stream);

#endif /* PGR_MATCH_H_ABI */
