/*
 * pgr.h -- C ABI of the MI355X-native pygenray hot path (libpgr_hip.so).
 *
 * pygenray has no FFI/plugin interface; the seam this library slots into is the
 * array-level contract pygenray itself uses to cross its process boundary
 * (REF = /root/reference/src/pygenray):
 *
 *   - the 7 environment arrays  cin, cpin, rin, zin, depths, depth_ranges,
 *     bottom_angle                      REF/multi_processing.py:37-45,90
 *   - per-ray y0 = [T0, z0, p0] + scalars, i.e. the argument list of
 *     _shoot_single_ray_process / _shoot_ray_array
 *                                       REF/launch_rays.py:487-497, 325-340
 *   - per-ray result [r; T; z; p] on linspace(source_range, receiver_range,
 *     num_range_save) + n_bottom, n_surface, or "None" for a dropped ray
 *                                       REF/launch_rays.py:561-576, 745-784
 *
 * Everything is plain pointers and sizes: no torch / HIP types in signatures
 * (a HIP stream is passed as void*).  All floating point is IEEE binary64.
 * Values are in the ODE convention (depth positive down); the caller applies
 * pygenray's storage sign flip z -> -z, p -> -p (REF/ray_objects.py:51-52).
 *
 * Return value of every int function: 0 = success, <0 = error (see
 * pgr_last_error()).  No exception or signal crosses this boundary; per-ray
 * failures are reported in status[] (pygenray swallows them and drops the
 * ray, REF/launch_rays.py:578-581).
 */
#ifndef PGR_H
#define PGR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* per-ray status codes (status[k]) */
#define PGR_RAY_OK 0             /* reached receiver_range */
#define PGR_RAY_VERTICAL 1       /* vertical_ray event      REF/launch_rays.py:443-448 */
#define PGR_RAY_BBOX 2           /* left the c(r,z) table    REF/launch_rays.py:451-456 */
#define PGR_RAY_BACKWARD 3       /* |theta_bounce| > 90      REF/launch_rays.py:474-477 */
#define PGR_RAY_STEP_TOO_SMALL 4 /* solve_ivp status -1      REF/launch_rays.py:427-430 */
#define PGR_RAY_MAX_STEPS 5      /* guard: max_steps accepted steps exceeded (no reference counterpart) */
#define PGR_RAY_BETA_RANGE 6     /* bottom-angle interp1d out of bounds (ValueError) REF/launch_rays.py:469 */
#define PGR_RAY_EVENT_ERROR 7    /* event root not bracketed (brentq ValueError) */
#define PGR_RAY_SKIPPED 8        /* not integrated: PGR_SKIP_NAN_Y0 and a NaN initial slowness (a finished eigenray bracket) */

/* flags for pgr_shoot_fan* */
#define PGR_TERMINATE_BACKWARDS 1u /* REF/launch_rays.py:19,474 (default True) */
#define PGR_SAMPLE_MAJOR 2u        /* T/z/p laid out [S][N] instead of [N][S] */
#define PGR_EXACT_BISECTION 4u     /* locate events with brentq's ~42-step bisection, the true +-1 event evaluated
                                      at every iterate (SCIPY/ivp.py:51-76), instead of the default replay of the
                                      same iterates that evaluates it only inside the rounding-noise band around
                                      the root: the same root either way */

#define PGR_SAVE_LINSPACE 8u       /* (device entry) the caller asserts r_save is exactly
                                      np.linspace(source_range, receiver_range, S); the kernel then
                                      recomputes r_save[j] = j*step + start instead of loading it.
                                      The host entry sets/clears this bit itself after checking. */
#define PGR_DEBUG_TRIPS 16u       /* diagnostics: n_rej[] receives, per wave, the number of main-loop
                                      trips (lane 0), of service phases (lane 1) and, per ray, how often
                                      the exact event bisection ran (lanes 2..63) instead */

#define PGR_EXACT_SAMPLES 32u      /* evaluate the saved samples with SciPy's own summation order
                                      (Q = K.T @ P, then h * (Q @ p) + y_old, SCIPY/rk.py:552-574)
                                      instead of the default stage-major FMA form of the same quartic
                                      (a few ulp apart; samples never feed back into the integration) */

#define PGR_STORED_SIGN 64u        /* T/z/p trajectories in pygenray's stored convention: z -> -z,
                                      p -> -p (REF/ray_objects.py:51-52); end_state stays ODE-signed */

#define PGR_COMPACT 128u           /* (host entry, with PGR_SAMPLE_MAJOR) dropped rays vanish from the
                                      trajectories as they do from a pygenray RayFan
                                      (REF/launch_rays.py:166-171): T/z/p come back as [S][M], M = number
                                      of rays with status 0, in launch order, at the start of the caller's
                                      [S][N] buffers; the per-ray arrays keep all N entries */

#define PGR_PACKED_END 256u        /* (device entry) end_state is [N][5] doubles: T, z, p, then n_bott,
                                      n_surf, status and a valid mark (1) as four int32 in the last two
                                      slots -- the end record the multi-GPU all-gather ships, written by
                                      the kernel instead of packed afterwards */

#define PGR_SAMPLE_BLOCKED 2048u   /* (with PGR_SAMPLE_MAJOR; environments whose tables stay in HBM / L2) T / z / p are written as
                                     [ceil(S / 4)][N][4]: sample j of ray k at ((j / 4) * N + k) * 4 + j % 4 -- every lane stages four
                                     consecutive samples in LDS and stores them as one full 32-byte piece per array.  The buffers hold
                                     4 * ceil(S / 4) * N doubles (rows S ... 4 * ceil(S / 4) - 1 are padding).  pgr_shoot_fan_device only
                                     (a layout for device-resident consumers), with PGR_SAVE_LINSPACE and the default sample form; an
                                     error for environments on the LDS-table path and in the host-pointer / fan-handle entries. */
#define PGR_LAUNCH_SLOWNESS 1024u   /* (pgr_fan_launch without y0) the array of launch angles holds the initial vertical
                                      slowness p0[k] = sin(radians(angle_k)) / c_source itself, computed by the caller
                                      (REF/launch_rays.py:144): y0[k] = [0, source_depth, p0[k]] is assembled on the device */

#define PGR_SKIP_NAN_Y0 512u       /* rays whose y0[k][2] is NaN are not integrated (status PGR_RAY_SKIPPED): the
                                      eigenray refinement parks its finished brackets this way */

typedef struct pgr_env pgr_env; /* opaque: environment tables resident in HBM */

/* Number of visible HIP devices (<0 on error). */
int pgr_device_count(void);

/* Upload one environment (the 7-array contract, REF/multi_processing.py:37-45) to
 * `device`.  Replaces _init_shared_memory/_unpack_shared_memory: one H2D copy instead of
 * 7 POSIX shm blocks.  cin/cpin are [nr][nz] C-contiguous (range-major), bottom_angles in
 * degrees.  Coordinates must be non-decreasing (REF/launch_rays.py:79-90) and nb >= 4
 * (cubic interp1d, REF/launch_rays.py:397-399).  Host buffers stay owned by the caller. */
int pgr_env_create(pgr_env** env, int device, const double* cin, const double* cpin,
                   const double* rin, const double* zin, int64_t nr, int64_t nz,
                   const double* depths, const double* depth_ranges, const double* bottom_angles,
                   int64_t nb);
/* Releases the tables, workspaces and stream.  While device-resident fans (pgr_fan_launch below) of this
 * environment are alive the release is deferred to the pgr_fan_destroy of the last of them; the handle must not be
 * used for new calls after pgr_env_destroy either way. */
void pgr_env_destroy(pgr_env* env);

/* Properties the kernel selection depends on (for tests / diagnostics):
 * what = 0: tables range independent (all rows bitwise equal) ; 1: zin exactly uniform ;
 *        2: rin exactly uniform ; 3: LDS-resident table path selected ; 4: device index ;
 *        5 / 6 / 7: zin qualifies for the cubic index estimate / the quadratic one / the bin table ;
 *        8: a sample-major trajectory fan of this environment is best written PGR_SAMPLE_BLOCKED (tables in HBM / L2, LDS left
 *           for the staging, PGR_OPT_API_BLOCKED on): what pgr_shoot_fan / pgr_fan_launch do by themselves and what a
 *           device-resident consumer of pgr_shoot_fan_device should ask for (the Python DeviceFan does by default). */
int pgr_env_query(const pgr_env* env, int what);

/* Shoot N rays: batched _shoot_ray_array + _interpolate_ray (REF/launch_rays.py:325-484,
 * 745-784) with SciPy's RK45 defaults (REF/launch_rays.py:670-679: rtol given, atol 1e-6,
 * dense output, 4 terminal events).
 *
 *   rtol, atol    as solve_ivp takes them: rtol > 0 (below 100 EPS it is raised to 100 EPS, SCIPY/common.py:44-51),
 *                 atol >= 0
 *   y0[N][3]      initial [T, z, p]   (REF/launch_rays.py:140-144)
 *   r_save[S]     np.linspace(source_range, receiver_range, S), computed by the caller
 *   T,z,p         [N][S] (or [S][N] with PGR_SAMPLE_MAJOR); may all be NULL = end state only.
 *                 Rays with status != 0 are filled with NaN.
 *   end_state     [N][3] exact final [T,z,p] (= last column), may be NULL
 *   n_bott,n_surf [N] bounce counts ; status [N] ; n_steps [N] accepted RK45 steps ;
 *   n_rej [N] rejected attempts (n_steps/n_rej may be NULL)
 *
 * pgr_shoot_fan takes HOST pointers (copies in/out, synchronous): everything it does is enqueued on a
 * stream owned by `env` and it waits for that stream only; calls on one env are serialised.
 * pgr_shoot_fan_device takes DEVICE pointers on env's device, enqueues on `stream`
 * (hipStream_t as void*, NULL = default stream) and returns without synchronising. */
int pgr_shoot_fan(pgr_env* env, const double* y0, int64_t N, double source_range,
                  double receiver_range, const double* r_save, int32_t S, double rtol, double atol,
                  uint32_t flags, int64_t max_steps, double* T, double* z, double* p,
                  double* end_state, int32_t* n_bott, int32_t* n_surf, int32_t* status,
                  int32_t* n_steps, int32_t* n_rej);
int pgr_shoot_fan_device(pgr_env* env, const double* y0, int64_t N, double source_range,
                         double receiver_range, const double* r_save, int32_t S, double rtol,
                         double atol, uint32_t flags, int64_t max_steps, double* T, double* z,
                         double* p, double* end_state, int32_t* n_bott, int32_t* n_surf,
                         int32_t* status, int32_t* n_steps, int32_t* n_rej, void* stream);

/* Initial states on the device (REF/launch_rays.py:140-144, 284-285): y0[k] = [0, source_depth,
 * sin(radians(ode_angles_deg[k])) / c_source], the sine correctly rounded (the arithmetic pgr_eigen_refine uses for its
 * trial rays); DEVICE pointers, enqueued on `stream`, returns without synchronising.  c_source = c at the source (the
 * caller's bilinear_interp, REF/launch_rays.py:140). */
int pgr_initial_states_device(int device, const double* ode_angles_deg, int64_t N, double source_depth,
                              double c_source, double* y0, void* stream);

/* A fan whose results stay in HBM.  pgr_fan_launch uploads y0[N][3] (HOST) -- or, when y0 is NULL, the N ODE launch
 * angles ode_angles_deg (HOST, degrees), from which the initial states are computed on the device as above --
 * enqueues the fan on the environment's stream and returns as soon as the upload is done: the kernel is still running.
 * S = num_range_save of the trajectories kept on the device ([S][N], the save grid is np.linspace(source_range,
 * receiver_range, S)); S = 0: end states only.  flags as pgr_shoot_fan (PGR_TERMINATE_BACKWARDS, PGR_EXACT_*,
 * PGR_STORED_SIGN).  pgr_fan_wait blocks until the kernel has finished and tells the ray count and how many have
 * status 0.  pgr_fan_fetch_rays copies the per-ray arrays ([N], any may be NULL) to HOST buffers; pgr_fan_fetch_samples
 * copies the trajectories asked for (T, z, p: HOST [S][N], any may be NULL; with PGR_COMPACT [S][M], dropped rays
 * squeezed out as in a pygenray RayFan, REF/launch_rays.py:166-171) -- page faults of fresh destination buffers
 * pipelined with the copies.  Both wait for the kernel themselves.  What pygenray's RayFan holds as host arrays
 * (REF/launch_rays.py:166-186) crosses PCIe only when somebody asks for it. */
typedef struct pgr_fan pgr_fan;
int pgr_fan_launch(pgr_env* env, const double* y0, const double* ode_angles_deg, double source_depth, double c_source,
                   int64_t N, double source_range, double receiver_range, int32_t S, double rtol, double atol,
                   uint32_t flags, int64_t max_steps, pgr_fan** fan);
int pgr_fan_wait(pgr_fan* fan, int64_t* n_rays, int64_t* n_ok);
int pgr_fan_fetch_rays(pgr_fan* fan, double* end_state, int32_t* n_bott, int32_t* n_surf, int32_t* status,
                       int32_t* n_steps, int32_t* n_rej);
int pgr_fan_fetch_samples(pgr_fan* fan, double* T, double* z, double* p, uint32_t flags);
/* The per-ray results of the M surviving rays only, in launch order (what a pygenray RayFan keeps): end_state [M][3],
 * n_bott / n_surf [M] as int64; per_ray_in [N] -> per_ray_out [M] squeezes any per-ray HOST array of the caller's
 * (the stored launch angles) the same way.  Any pair may be NULL.  M from pgr_fan_wait. */
int pgr_fan_fetch_rays_compact(pgr_fan* fan, const double* per_ray_in, double* per_ray_out, double* end_state,
                               int64_t* n_bott, int64_t* n_surf);
void pgr_fan_destroy(pgr_fan* fan);

/* Eigenray refinement: pygenray's _find_single_eigenray (REF/eigenrays.py:206-268) for nbk brackets at
 * once, the whole false-position loop on the device.  Per bracket k the fan rays th1[k], th2[k] (user
 * launch angles, degrees) ended at stored-convention depths z1[k], z2[k] on either side of
 * -receiver_depth.  Each iteration is: trial angle (REF/eigenrays.py:118-120, 261-263) and its initial
 * state y0 = [0, source_depth, sin(radians(-theta)) / c_source] (REF/launch_rays.py:251,284-285; the
 * sine correctly rounded) in one small kernel, ONE fan launch (end state only) over all brackets still
 * active (the others are skipped in place, PGR_SKIP_NAN_Y0), the update of the reference's loop in the
 * next small kernel: dropped ray -> failed; |z_end + receiver_depth| < ztol -> found; else the trial ray
 * replaces the bracket end on its side; give up after max_iter + 2 trial rays (REF/eigenrays.py:265-268).
 * Everything is enqueued on the environment's stream; the host only reads back the count of active
 * brackets after each iteration.  HOST arrays in and out:
 *   theta[k]  state 1: the eigenray's launch angle (user convention); state 2: the angle of the trial ray that was
 *   dropped (what the reference prints in its failure message); state 3: the next trial angle the loop would have
 *   shot;   state[k]  1 found, 2 trial ray dropped (the reference prints "Failed to find eigen ray" and gives
 *   up), 3 iteration limit;
 *   n_trial[k] trial rays shot;  z_end[k], t_end[k] stored-convention end depth / arrival time of the
 *   last trial ray.  *launches = fan launches made.  c_source = c at the source (the caller's
 *   bilinear_interp, REF/launch_rays.py:284). */
int pgr_eigen_refine(pgr_env* env, int64_t nbk, const double* th1, const double* th2, const double* z1,
                     const double* z2, double receiver_depth, double source_depth, double source_range,
                     double receiver_range, double c_source, double rtol, double atol, uint32_t flags,
                     int64_t max_steps, double ztol, int32_t max_iter, double* theta, int32_t* state,
                     int32_t* n_trial, double* z_end, double* t_end, int32_t* launches);
/* The same search with a receiver depth per bracket, receiver_depths[nbk]: find_eigenrays loops over its receiver
 * depths (REF/eigenrays.py:62) and searches the brackets of each; an iteration of the device loop lasts as long as
 * its slowest trial ray whatever the number of brackets, so the brackets of ALL receiver depths iterate together --
 * R depths cost one search instead of R.  Same results, bracket by bracket, as R calls of pgr_eigen_refine. */
int pgr_eigen_refine_depths(pgr_env* env, int64_t nbk, const double* th1, const double* th2, const double* z1,
                            const double* z2, const double* receiver_depths, double source_depth, double source_range,
                            double receiver_range, double c_source, double rtol, double atol, uint32_t flags,
                            int64_t max_steps, double ztol, int32_t max_iter, double* theta, int32_t* state,
                            int32_t* n_trial, double* z_end, double* t_end, int32_t* launches);

/* ... and with the trial rays' initial slowness computed by the CALLER: `slowness(ode_angles_deg, n, p0_out, user)` must set
 * p0_out[k] = sin(radians(ode_angles_deg[k])) / c_source for k < n (HOST arrays; a NaN angle -- a finished bracket -- must give
 * a NaN) with the caller's own sine.  pygenray computes every initial slowness with NumPy's sine (REF/launch_rays.py:284-285),
 * which is faithful, not correctly rounded: the Python shim passes NumPy's here, so that a trial ray, the eigenray handed back and
 * shoot_ray(theta) of the same angle all start from the SAME bits, the reference's.  Costs one small D2H + H2D per iteration.
 * slowness == NULL: the device's correctly rounded sine, as pgr_eigen_refine_depths.
 * The callback runs on the calling thread INSIDE the search: the environment's workspace lock is held and its buffers are in
 * use, so it must NOT call back into the same environment: pgr_shoot_fan, pgr_eigen_refine*, pgr_fan_*, pgr_env_destroy on `env`
 * would deadlock or reallocate the workspace under the loop; other environments are fine.  It must not throw / longjmp
 * through the C frames. */
typedef void (*pgr_slowness_fn)(const double* ode_angles_deg, int64_t n, double* p0_out, void* user);
int pgr_eigen_refine_depths_fn(pgr_env* env, int64_t nbk, const double* th1, const double* th2, const double* z1,
                               const double* z2, const double* receiver_depths, double source_depth, double source_range,
                               double receiver_range, double c_source, double rtol, double atol, uint32_t flags,
                               int64_t max_steps, double ztol, int32_t max_iter, double* theta, int32_t* state,
                               int32_t* n_trial, double* z_end, double* t_end, int32_t* launches,
                               pgr_slowness_fn slowness, void* slowness_user);

/* Arrival-time histogram of a fan's surviving rays on the device (BASELINE configs[4]; the
 * reduction behind pygenray's time-front scatter RayFan.plot_time_front, REF/ray_objects.py:157-222;
 * no reference counterpart for the binning itself, so it is NumPy's):
 * counts[nbins] (DEVICE, int64, overwritten) = np.histogram(T, bins=nbins, range=(t_min, t_max))[0]
 * over the rays k < N with status[k * status_stride] == 0 (status may be NULL = all rays) and T =
 * t_end[k * t_stride] not NaN; t_end / status are DEVICE pointers on `device`: e.g. end_state with
 * t_stride 3, or the packed end records (PGR_PACKED_END) with t_stride 5 and (int32*)(rec + 4) with
 * status_stride 10.  Enqueued on `stream`, returns without synchronising; every rank of a sharded
 * fan then all-reduces its counts.  nbins <= 16384. */
int pgr_arrival_histogram_device(int device, const double* t_end, int64_t t_stride,
                                 const int32_t* status, int64_t status_stride, int64_t N,
                                 double t_min, double t_max, int32_t nbins, int64_t* counts,
                                 void* stream);

/* Ray-tube intensity of a fan on a range-depth grid (the transmission loss of DESIGN.md, "Transmission loss"): adjacent
 * surviving rays k, k + 1 (launch order) bound a tube; at save sample s, with g = c / sqrt(1 - (p c)^2) and c the bilinear
 * sound speed of the environment the fan was traced in,
 *   I_k(s) = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / (r_s |z_k+1 - z_k|),   r_s = |x_s - x_0|,
 * and out[j * S + s] (DEVICE, [n_depths][S], overwritten) = the sum, in increasing k starting from 0.0, of I_k(s) over the
 * tubes whose depth interval [min, max) of their two samples holds depths[j].  A tube with a NaN sample, |p c| >= 1 at
 * either end or z_k+1 == z_k adds nothing (a receiver no tube reaches gets 0); the column r_s == 0 is NaN.  Depths are
 * positive down.  Deterministic: no atomics, every receiver's sum is formed in tube order by one lane, so repeated calls
 * are bit-equal and equal the sequential sum.  TL = -10 log10(out).
 *
 * pgr_fan_intensity: a device-resident fan (either trajectory layout it holds; dropped rays are skipped in place, nothing
 * is copied or fetched).  Waits for the fan's kernel, then enqueues on `stream` and returns without synchronising.
 * p0[M] (DEVICE): the launch slowness of the M surviving rays in launch order (only |p0_k+1 - p0_k| enters); depths[n_depths]
 * (DEVICE).  Needs M >= 2 and a fan launched with trajectories.  Sample depths are read as launched (PGR_STORED_SIGN:
 * depth = -z). */
int pgr_fan_intensity(pgr_fan* fan, const double* p0, const double* depths, int64_t n_depths, double* out, void* stream);

/* The same for caller buffers: z, p (DEVICE) [n_samples][n_rays] rows, stored sign convention (depth = -z, as RayFan.zs),
 * every ray a tube edge; x[n_samples] (DEVICE) the save ranges in the frame of `env` (mirrored, x -> -x, for a backwards fan);
 * p0[n_rays], depths[n_depths], out[n_depths][n_samples] as above.  Enqueued on `stream`, returns without synchronising. */
int pgr_intensity_device(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                         const double* x, const double* p0, const double* depths, int64_t n_depths, double* out,
                         void* stream);

/* Ray-tube arrivals at receiver depths ("Arrivals"): every tube k that pgr_fan_intensity adds at receiver j
 * and save column s -- the same validity and [lo, hi) tests, none added, none left out -- is one arrival, with
 *   w = (D_j - d_k) / (d_k+1 - d_k),   T = T_k + w (T_k+1 - T_k),   p = p_k + w (p_k+1 - p_k)   (p: stored sign),
 * I = the tube's term of the intensity sum (the same bits) and tube = k (rays k, k + 1 of the surviving rays).
 * cols[n_cols] (HOST, int32, each 0 .. S - 1, repeats allowed, 1 <= n_cols <= 65535): the columns asked for, slot c being
 * column cols[c].  The column r_s == 0 has no arrivals.  Two calls with the same arguments:
 *
 * pgr_fan_arrival_counts: counts[j * n_cols + c] (DEVICE int64, [n_depths][n_cols], overwritten) = the arrivals of
 *   receiver j at slot c.
 * pgr_fan_arrivals: offsets[j * n_cols + c] (DEVICE int64) = where those arrivals start, the exclusive scan of the counts;
 *   each receiver's arrivals at each slot are written there in increasing k into tube (int32), w, T, p, I (DEVICE,
 *   n_arrivals >= 1 entries each; nothing is written at or past n_arrivals).
 *
 * Deterministic: no atomics, one lane finds and writes one receiver's arrivals in tube order.  Fan arguments, waiting and
 * streams as pgr_fan_intensity. */
int pgr_fan_arrival_counts(pgr_fan* fan, const double* p0, const double* depths, int64_t n_depths, const int32_t* cols,
                           int32_t n_cols, int64_t* counts, void* stream);
int pgr_fan_arrivals(pgr_fan* fan, const double* p0, const double* depths, int64_t n_depths, const int32_t* cols,
                     int32_t n_cols, const int64_t* offsets, int64_t n_arrivals, int32_t* tube, double* w, double* T,
                     double* p, double* I, void* stream);

/* The same for caller buffers, as pgr_intensity_device: T, z, p (DEVICE) [n_samples][n_rays] rows, stored sign
 * convention, every ray a tube edge; x[n_samples] (DEVICE) the save ranges in the frame of `env`.  The counts need no T. */
int pgr_arrival_counts_device(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                              const double* x, const double* p0, const double* depths, int64_t n_depths,
                              const int32_t* cols, int32_t n_cols, int64_t* counts, void* stream);
int pgr_arrivals_device(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                        int32_t n_samples, const double* x, const double* p0, const double* depths, int64_t n_depths,
                        const int32_t* cols, int32_t n_cols, const int64_t* offsets, int64_t n_arrivals, int32_t* tube,
                        double* w, double* T_out, double* p_out, double* I, void* stream);

/* Incoherent geometric Gaussian-beam intensity of a fan on a range-depth grid ("Gaussian beams"): the tubes of
 * pgr_fan_intensity, each spread over depth as a Gaussian instead of a top hat.  At save sample s, tube k (rays k, k + 1)
 * with both g finite (no NaN sample, |p c| < 1 at both ends; equal depths allowed) has
 *   E_k = 0.5 (g_k + g_k+1) |p0_k+1 - p0_k| / r_s,   m_k = 0.5 (d_k + d_k+1),   A_k = E_k / (sigma_k sqrt(2 pi)),
 *   sigma_k = max(D_k-1, D_k, D_k+1, min_width),   D_i = |d_i+1 - d_i|   (NaN widths and those past the fan's ends ignored),
 * and out[j * S + s] (DEVICE, [n_depths][S], overwritten) = the sum, in increasing k from 0.0 and for each tube over the
 * centres m_k, -m_k and 2 bottom[s] - m_k in that order (the beam and its images in the surface and the bottom), of
 *   A_k exp(-v / 2),   v = ((depths[j] - centre) / sigma_k)^2,   over the terms with v <= 16 (beams cut at 4 sigma).
 * exp is a fixed sequence of + - x, rint and ldexp (the library's own, within 1.5 ulp on [-8, 0]).  A receiver no beam
 * reaches gets 0; the column r_s == 0 is NaN.  Deterministic: no atomics, every receiver's sum is formed in order by one
 * lane, so repeated calls are bit-equal and equal the sequential sum.  TL = -10 log10(out).
 *
 * bottom[S] (DEVICE): the bottom depth at each save range, in the frame the fan was traced in (flat-earth, mirrored for a
 * backwards fan).  min_width: the floor on sigma, metres, finite and > 0.
 * pgr_fan_beam_intensity: a device-resident fan, with the fan arguments, waiting and streams of pgr_fan_intensity.
 * pgr_beam_intensity_device: caller buffers z, p (DEVICE) [n_samples][n_rays] rows, stored sign convention, and x as
 * pgr_intensity_device. */
int pgr_fan_beam_intensity(pgr_fan* fan, const double* p0, const double* bottom, const double* depths, int64_t n_depths,
                           double min_width, double* out, void* stream);
int pgr_beam_intensity_device(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                              const double* x, const double* p0, const double* bottom, const double* depths,
                              int64_t n_depths, double min_width, double* out, void* stream);

/* Travel-time sensitivity kernel of a fan on a range-depth grid ("Travel-time sensitivity kernels"): the linear
 * map dT = K . dc from a sound-speed perturbation on the grid ranges[n_ranges] x depths[n_depths] to the travel times of
 * the surviving rays at save column `column`.  Per ray m (depth d = -z, travel time T, save ranges x), the path is the
 * polyline through samples 0 ... column; chord s -> s + 1 is cut at every interior grid line it crosses strictly inside,
 * and each piece (length l, in the grid cell it lies in) adds, by Simpson's rule at its ends and midpoint,
 *   Q_ab(s) += l/6 [f(0) + 4 f(1/2) + f(1)],  f = phi_ab / c^2,       Q_1(s) += l/6 [g(0) + 4 g(1/2) + g(1)],  g = 1 / c,
 * phi_ab the bilinear weight of node (a, b) (host_physics.bilinear_interp: clamped cell, unclamped weights), c the
 * look-up of pgr_fan_intensity.  Then
 *   out[(m * n_ranges + a) * n_depths + b] = sum over s < column, in increasing s from 0.0, of
 *                                            - beta_s Q_ab(s),   beta_s = (T(s+1) - T(s)) / Q_1(s)  (0 if Q_1 == 0),
 * in s / (m/s).  A NaN in T or z at samples 0 ... column makes row m all NaN; column 0 gives zeros.  Divisions and the
 * square root correctly rounded, nothing contracted (reference build).  Every entry is written (zeros included); no
 * atomics: one lane forms each entry in the order above, so repeated calls are bit-equal.
 *
 * ranges[n_ranges], depths[n_depths] (DEVICE): strictly ascending, 2 <= n_ranges <= 65535, 2 <= n_depths <= 2^30; the
 * ranges in the frame the fan was traced in (mirrored, x -> -x and reversed, for a backwards fan).  out (DEVICE)
 * [M][n_ranges][n_depths] float64.  0 <= column < n_samples.
 * pgr_fan_travel_time_kernel: a device-resident fan with the fan arguments, waiting and streams of pgr_fan_intensity
 *   (either trajectory layout, dropped rays skipped through the keep list); M = its surviving rays, at least 1.
 * pgr_travel_time_kernel_device: caller buffers T, z (DEVICE) [n_samples][n_rays] rows, stored sign convention, every ray
 *   kept (M = n_rays, at most 2^24), x[n_samples] (DEVICE) the save ranges in the frame of `env`.  Enqueued on `stream`,
 *   returns without synchronising. */
int pgr_fan_travel_time_kernel(pgr_fan* fan, const double* ranges, int32_t n_ranges, const double* depths, int32_t n_depths,
                               int32_t column, double* out, void* stream);
int pgr_travel_time_kernel_device(pgr_env* env, const double* T, const double* z, int64_t n_rays, int32_t n_samples,
                                  const double* x, const double* ranges, int32_t n_ranges, const double* depths,
                                  int32_t n_depths, int32_t column, double* out, void* stream);

/* Time fronts and turning-point counts of a fan at chosen save columns ("Time fronts and ray
 * identifiers").  For surviving ray m (launch order) with slowness samples p_m(s), s = 0 ... S - 1, let cls(v) = +1 for
 * v > 0, -1 for v < 0, 0 for v == +-0, a NaN being a class that differs from every class, itself included.  Then
 *   change_m(s) = 1 if cls(p_m(s + 1)) differs from cls(p_m(s)) else 0,        s = 0 ... S - 2,
 *   turns[c * M + m] (DEVICE int32, [n_cols][M], overwritten) = sum over s < cols[c] of change_m(s)   (0 for column 0),
 * entry for entry np.sum(np.diff(np.sign(ps[:, :col + 1]), axis=1) != 0, axis=1): the reference's ray-identifier count
 * (REF/ray_objects.py:142) of the path up to column col, the same in either sign convention of p.  T_out, z_out, p_out
 * (DEVICE float64, [n_cols][M] each, overwritten) = T, z, p of the surviving rays at column cols[c], the bits the fan holds.
 * Any of the four outputs may be NULL, not all.  cols[n_cols] (HOST, int32, each 0 .. S - 1, repeats and any order allowed,
 * 1 <= n_cols <= 65535): slot c is column cols[c].  An integer prefix sum: no atomics, and the same answer in any order;
 * p is read up to max(cols) only (each sample once, plus one seam sample per segment of at most 32).
 *
 * pgr_fan_time_front: a device-resident fan (either trajectory layout it holds; dropped rays are skipped in place, nothing
 *   is copied or fetched).  Waits for the fan's kernel, then enqueues on `stream` and returns without synchronising.  Needs
 *   M >= 1 and a fan launched with trajectories.
 * pgr_time_front_device: caller buffers T, z, p (DEVICE) [n_samples][n_rays] rows on `device`, every ray kept
 *   (M = n_rays); an input may be NULL when its output is NULL, p is needed for turns as well.  Enqueued on `stream`,
 *   returns without synchronising. */
int pgr_fan_time_front(pgr_fan* fan, const int32_t* cols, int32_t n_cols, double* T_out, double* z_out, double* p_out,
                       int32_t* turns, void* stream);
int pgr_time_front_device(int device, const double* T, const double* z, const double* p, int64_t n_rays,
                          int32_t n_samples, const int32_t* cols, int32_t n_cols, double* T_out, double* z_out,
                          double* p_out, int32_t* turns, void* stream);

/* Running path integral of every ray of a fan at every save range ("Path integrals and volume
 * absorption").  For surviving ray m (launch order) with samples s = 0 ... S - 1: depth d_s (= -z in the stored convention),
 * travel time T_s, save range x_s in the frame the fan was traced in, c_s the bilinear sound speed of pgr_fan_intensity at
 * (x_s, d_s), and alpha_s = alpha(d_s) from the profile alpha[n_a] (dB per metre, finite, >= 0) at the strictly ascending
 * depth nodes a_depths[n_a] (metres, positive down, the frame's depths):
 *   n_a == 1: alpha_s = alpha[0] (a_depths may be NULL);
 *   else alpha[0] for d_s <= a_depths[0], alpha[n_a - 1] for d_s >= a_depths[n_a - 1], and in between, with the cell
 *   j = np.searchsorted(a_depths, d_s, side="right") - 1 clamped to 0 ... n_a - 2,
 *   alpha_j + w (alpha_j+1 - alpha_j),  w = (d_s - a_depths_j) / (a_depths_j+1 - a_depths_j);  NaN for a NaN depth.
 * Then, with q_s = alpha_s c_s,
 *   inc_s = (0.5 (q_s + q_s+1)) (T_s+1 - T_s)   [dB],   s = 0 ... S - 2   (the trapezoid rule on ds = c dT),
 *   out[0 * M + m] = 0.0,   out[(s + 1) * M + m] = out[s * M + m] + inc_s   sequentially, in increasing s.
 * out (DEVICE, float64 [S][M], rows over the SURVIVING rays whatever the fan's own layout; every entry is written).  A NaN in
 * T or d propagates by IEEE rules: the ray's entries are NaN from that sample on (entry 0 is 0.0 regardless).  The division
 * is correctly rounded and nothing is contracted (reference build).  alpha == {1.0}: the path length in metres -- in the
 * traced frame: for a flat-earth environment the flat-earth length, which exceeds the true one by a factor of at most
 * exp(z / R_earth), about 1 + 8e-4 at 5 km.  No atomics: one lane forms each ray's sums in the order above, so repeated calls
 * are bit-equal and equal the sequential sum.
 *
 * a_depths, alpha are HOST arrays, checked before any device work (n_a < 1, nodes that are not finite or do not ascend, an
 * alpha that is not finite or negative and NULL pointers are errors, and nothing is written).
 * pgr_fan_path_integral: a device-resident fan (either trajectory layout it holds; dropped rays are skipped in place, nothing
 *   is copied or fetched).  Waits for the fan's kernel, then enqueues on `stream` and returns without synchronising.  Needs
 *   M >= 1 and a fan launched with trajectories.
 * pgr_path_integral_device: caller buffers T, z (DEVICE) [n_samples][n_rays] rows, stored sign convention, every ray kept
 *   (M = n_rays), x[n_samples] (DEVICE) the save ranges in the frame of `env`. */
int pgr_fan_path_integral(pgr_fan* fan, const double* a_depths, const double* alpha, int32_t n_a, double* out, void* stream);
int pgr_path_integral_device(pgr_env* env, const double* T, const double* z, int64_t n_rays, int32_t n_samples,
                             const double* x, const double* a_depths, const double* alpha, int32_t n_a, double* out,
                             void* stream);

/* The weights volume absorption gives the tube products: W[i] = 10^(-A[i] / 10) for a path integral A in dB (DEVICE, n
 * entries each; W may be A itself), computed as exp(y), y = -(A[i] K), K = 0x1.d791c5f888822p-3 the double nearest
 * ln(10) / 10, with the library's own exp of pgr_fan_beam_intensity (a fixed sequence of + - x, rint and ldexp; within
 * 1.5 ulp on [-700, 0]); 0.0 for y < -700 and NaN for a NaN.  Enqueued on `stream`, returns without synchronising. */
int pgr_absorption_weights_device(int device, const double* A, int64_t n, double* W, void* stream);

/* Weighted twins of the tube entries: the same calls with `weights` (DEVICE, float64 [S][M] rows over the surviving rays,
 * as pgr_fan_path_integral writes them; [n_samples][n_rays] for the _device entries), after which every g of the
 * definitions above is g W[s * M + m] -- so I_k = 0.5 (g_k W_k + g_k+1 W_k+1) |dp0| / (r |dz|), the beams' E_k likewise, and
 * an arrival's I is the weighted tube's.  Validity tests and the intervals [lo, hi) are those of the unweighted calls, so
 * the tubes counted, their order and pgr_fan_arrival_counts / pgr_arrival_counts_device are unchanged by finite weights
 * (there is no weighted count); a NaN weight makes its sample one that adds nothing, as a NaN sample does.  weights == NULL:
 * exactly the unweighted entry, which is this call with NULL (the same bits). */
int pgr_fan_intensity_w(pgr_fan* fan, const double* p0, const double* weights, const double* depths, int64_t n_depths,
                        double* out, void* stream);
int pgr_intensity_device_w(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                           const double* x, const double* p0, const double* weights, const double* depths,
                           int64_t n_depths, double* out, void* stream);
int pgr_fan_beam_intensity_w(pgr_fan* fan, const double* p0, const double* weights, const double* bottom,
                             const double* depths, int64_t n_depths, double min_width, double* out, void* stream);
int pgr_beam_intensity_device_w(pgr_env* env, const double* z, const double* p, int64_t n_rays, int32_t n_samples,
                                const double* x, const double* p0, const double* weights, const double* bottom,
                                const double* depths, int64_t n_depths, double min_width, double* out, void* stream);
int pgr_fan_arrivals_w(pgr_fan* fan, const double* p0, const double* weights, const double* depths, int64_t n_depths,
                       const int32_t* cols, int32_t n_cols, const int64_t* offsets, int64_t n_arrivals, int32_t* tube,
                       double* w, double* T, double* p, double* I, void* stream);
int pgr_arrivals_device_w(pgr_env* env, const double* T, const double* z, const double* p, int64_t n_rays,
                          int32_t n_samples, const double* x, const double* p0, const double* weights,
                          const double* depths, int64_t n_depths, const int32_t* cols, int32_t n_cols,
                          const int64_t* offsets, int64_t n_arrivals, int32_t* tube, double* w, double* T_out,
                          double* p_out, double* I, void* stream);

/* Tuning options of ONE environment (per-ray results never depend on them; there is no process-wide
 * state: host threads that drive different GPUs hold different environments).
 *   PGR_OPT_WAVES_PER_BLOCK  a = waves (of 64 rays) per workgroup, 0 = automatic
 *   PGR_OPT_DEPTH_SEARCH     depth-cell search for a non-uniform zin: a = 0 (default) from LDS -- when a cubic
 *                            in z estimates the node index to a small fraction of a cell (the flat-earth
 *                            transform of a uniform grid: 1.5e-8 cells), the cell is trunc(t(z)) or, rarely,
 *                            the next one, and two nodes are read; else the cell is j0 or j0 + 1 with j0 =
 *                            floor(g(z) - 0.5) from a quadratic estimate g (three nodes read), else j0 =
 *                            bucket[floor((z - z0)/w)] from a bin table; a = 1 always the binary search of
 *                            np.searchsorted (REF/integration_processes.py:152-157); a = 2 the bin table;
 *                            a = 3 the quadratic estimate (no cubic).  Tests compare the four.
 *   PGR_OPT_PARK             bounce-service batching: a wave services its parked (bounced) lanes when `a`
 *                            of them wait or the oldest waited `b` step attempts (default 64, 10)
 *   PGR_OPT_PLACEMENT        cost-aware wave scheduling for fans of 1-2 waves per SIMD: a = 2 (default) the
 *                            costliest waves get a SIMD to themselves / are paired with the cheapest, plus
 *                            issue priorities by cost quartile; 1 = priorities only; 0 = strided deal
 *   PGR_OPT_PERSISTENT       fans of several rounds (more 64-ray packets than the chip holds waves): a = 1 (default)
 *                            one workgroup per CU whose waves claim packet after packet from the cost-sorted list
 *                            (most expensive first) with one atomic each -- in fans of up to two rounds the first
 *                            packet of a workgroup's waves 4 .. 7 (the SIMD partners of waves 0 .. 3) comes from the
 *                            list's cheap end, so that every steep packet starts beside a cheap one; a = 2 / 3 never /
 *                            always so; a = 0 the static deal of whole cost-sorted workgroups (what replaces the
 *                            reference's pool.imap over single rays, REF/launch_rays.py:157-164, either way)
 *   PGR_OPT_API_BLOCKED      pgr_shoot_fan (sample-major) and pgr_fan_launch on environments whose tables stay in HBM / L2:
 *                            a = 1 (default) the trajectories are integrated by the sample-blocked kernel
 *                            (PGR_SAMPLE_BLOCKED: full 32-byte stores, 1.2x instead of 2.3x the sample bytes written) and
 *                            un-blocked to [S][M] by the pass that squeezes dropped rays out on the way to the host;
 *                            a = 0 plain [S][N] rows.  The caller sees the same arrays, bit for bit.
 *   PGR_OPT_D2H_REGISTER     the pipelined copy of large trajectory arrays (more than 32 MB in all) to the caller's pageable
 *                            buffers (pgr_shoot_fan, pgr_fan_fetch_samples): a = 1 (default) helper threads page-lock each
 *                            128 MiB sub-job (hipHostRegister) once its pages exist and the copy is one DMA into it; a = 0
 *                            never page-lock: every sub-job is copied piece by piece through the runtime's staging, which is
 *                            what a process under a locked-memory limit gets when the registration fails.  Same arrays,
 *                            bit for bit (tests/test_transfer.py runs both). */
#define PGR_OPT_WAVES_PER_BLOCK 0
#define PGR_OPT_DEPTH_SEARCH 1
#define PGR_OPT_PARK 2
#define PGR_OPT_PLACEMENT 3
#define PGR_OPT_PERSISTENT 4
#define PGR_OPT_API_BLOCKED 5
#define PGR_OPT_D2H_REGISTER 6
int pgr_env_set_option(pgr_env* env, int what, int a, int b);

/* Unit-level device entry points (for parity tests of a1-a8, REF/integration_processes.py):
 * evaluate on the GPU, for M query points (x[k], y[k][3]) given as HOST arrays:
 *   out[k][0..2] = derivsrd ; out[k][3] = bilinear c ; out[k][4] = ray angle (deg) ;
 *   out[k][5..8] = surface, bottom, vertical, bbox event values (+-1) ; out[k][9] = bathymetry
 *   linear_interp at x. */
int pgr_eval_points(pgr_env* env, const double* x, const double* y, int64_t M, double* out10);

/* Accuracy probe of the kernel's arithmetic building blocks (tests only): for HOST arrays a, b
 * of length M, out[k] = { a/b, 1/b, 1/sqrt(b), sqrt(b), b**-0.2, 10*ulp(a), b**0.2, asin(a), sin(a) }
 * as the kernel computes them (the last five of them correctly rounded, csrc/pgr_crmath.h). */
int pgr_debug_math(const double* a, const double* b, int64_t M, double* out9);

/* One RK45 step attempt per query (tests / debugging): for M HOST triples (t[k], y[k][3], h[k]) the
 * device evaluates f = derivsrd(t, y), rk_step (SCIPY/rk.py:14-71), the error norm (rk.py:106-110,
 * 146-147) and the controller's 0.9 * error_norm ** -0.2 with the fan kernel's own code:
 * out[k] = { y_new[3], f_new[3], error_norm, 0.9 err**-0.2, f[3] }. */
int pgr_debug_step(pgr_env* env, const double* t, const double* y, const double* h, int64_t M,
                   double rtol, double atol, double* out11);

/* Which instance of the fan kernel the LAST pgr_shoot_fan_device on `env` launched, and how (tests: the instance walk of
 * tests/test_hip_parity.py asserts that every instance it means to check is the one that ran):
 * out = { LDS_TAB, ZM, SAVE, PERSIST, grid (workgroups), threads per workgroup, dynamic LDS bytes, pre-assigned queue tail };
 * LDS_TAB: table in LDS (1) or HBM / L2 (0); ZM: depth look-up 0 division / binary search, 1 power-of-two dz, 2 bin table,
 * 3 quadratic estimate + three nodes, 4 dz = 1, 5 cubic estimate; SAVE: 0 end state, 1 trajectories (linspace grid, default sample
 * form), 2 any grid / PGR_EXACT_SAMPLES, 3 sample-blocked; PERSIST: persistent waves + packet queue.  -1s before any launch. */
int pgr_debug_last_instance(const pgr_env* env, int32_t out[8]);
/* LOG of that instance: 1 when it writes a bounce log (pgr_fan_launch_log), 0 when not; -1 before any launch or for a NULL env.
 * (An entry of its own: the eight slots above are taken.) */
int pgr_debug_last_instance_log(const pgr_env* env);

/* ---- The bounce log of a fan and boundary reflection loss ----
 *
 * pgr_fan_launch_log: pgr_fan_launch, whose arguments it takes, with a log of max_bounces (>= 1) slots per ray.  Whenever the
 * kernel applies a surface or bottom bounce to ray n, the ray's e-th (e = n_bott + n_surf before the bounce, counted from 0),
 * it writes slot [e][n] of three arrays the handle owns (pgr_fan_destroy frees them):
 *   bx (float64)  the range of the bounce: the located event abscissa, from which the next segment starts;
 *   bp (float64)  the slowness the next segment starts with, sin(radians(theta_bounce)) / c, in the sign of the fan's
 *                 trajectories (negated with PGR_STORED_SIGN);
 *   bk (int8)     0 surface, 1 bottom.
 * Events with e >= max_bounces are not written (n_bott / n_surf count on, so the overflow shows at the ray's end); slots never
 * written hold NaN, NaN, -1.  A bounce that ends the ray (bounced backwards, bottom angle outside the table) is not logged.
 * The integration never reads the log: status, counts, steps, end states and samples are those of pgr_fan_launch, bit for
 * bit.  Needs trajectories (num_range_save >= 1) without PGR_EXACT_SAMPLES, on an environment whose fans run the LDS-table
 * kernel or the sample-blocked one (PGR_OPT_API_BLOCKED on, the default); anything else is an error and nothing is launched.
 *
 * pgr_fan_fetch_bounces: bx, bp, bk (HOST, [max_bounces][M], NULL: not wanted) of the SURVIVING rays in launch order.  An
 * error on a fan without a log.
 *
 * pgr_fan_boundary_loss / pgr_boundary_loss_device: the loss in dB every ray has collected at its bounces up to every save
 * range.  For event e of ray m, with p = bp in the ODE sign (bp negated when stored):
 *   c_e     the bilinear sound speed of pgr_fan_intensity at (bx_e, d_b), d_b = 0 at the surface and, at the bottom, the
 *           environment's bottom depth at bx_e (linear in depths / depth_ranges, as the fan kernel evaluates it);
 *   theta_e = asin(p c_e) (correctly rounded) times 180 / pi;
 *   phi_e   = |theta_e| at the surface, |theta_e - beta(bx_e)| at the bottom, beta the table beta_deg on beta_x;
 *   loss_e  = the table bot_db on g_deg (bottom) or surf_db on s_deg (surface) at phi_e.
 * A table of n entries: n == 1 the constant (nodes may be NULL), else the interpolation rule of pgr_fan_path_integral (held
 * at the end values outside the strictly ascending nodes, linear with a correctly rounded weight in between).  A NaN in bx,
 * bp, theta (|p c| > 1) gives a NaN loss.  With x_s the save ranges np.linspace gives and E the ray's logged events (the
 * leading slots whose bk is not -1; their bx must not decrease, as a fan's do not):
 *   j_e = argmin_s |x_s - bx_e| (first minimum; 0 when bx_e is not finite),
 *   seg(s) = #{e < E : j_e <= s} for s < S - 1, seg(S - 1) = E     (the samples the reference's _interpolate_ray gives a segment),
 *   out_db[s * M + m] = sum of loss_e, e < seg(s), from 0.0 in increasing e;   nb / ns[s * M + m] = those events by kind.
 * out_db (DEVICE float64 [S][M]), nb, ns (DEVICE int32 [S][M], NULL: not wanted): every entry is written.  One lane forms each
 * ray's sum in order: no atomics, repeated calls are bit-equal.  The tables are HOST arrays, checked before any device work
 * (dB values finite and >= 0, beta finite, nodes finite and strictly ascending, n >= 1, out_db not NULL).  Enqueued on
 * `stream`; returns without synchronising.
 * pgr_fan_boundary_loss: a fan of pgr_fan_launch_log (waits for its kernel; dropped rays are skipped in place).
 * pgr_boundary_loss_device: caller buffers bx, bp, bk (DEVICE, [K][n_rays], stored sign, every ray kept) on the save ranges
 *   np.linspace(x0, x1, n_samples) in the frame of `env`. */
int pgr_fan_launch_log(pgr_env* env, const double* y0, const double* ode_angles_deg, double source_depth, double c_source,
                       int64_t N, double source_range, double receiver_range, int32_t num_range_save, double rtol,
                       double atol, uint32_t flags, int64_t max_steps, int32_t max_bounces, pgr_fan** out);
int pgr_fan_fetch_bounces(pgr_fan* fan, double* bx, double* bp, int8_t* bk);
int pgr_fan_boundary_loss(pgr_fan* fan, const double* g_deg, const double* bot_db, int32_t n_bot, const double* s_deg,
                          const double* surf_db, int32_t n_surf_tab, const double* beta_x, const double* beta_deg,
                          int32_t n_beta, double* out_db, int32_t* nb, int32_t* ns, void* stream);
int pgr_boundary_loss_device(pgr_env* env, const double* bx, const double* bp, const int8_t* bk, int64_t n_rays, int32_t K,
                             double x0, double x1, int32_t n_samples, const double* g_deg, const double* bot_db,
                             int32_t n_bot, const double* s_deg, const double* surf_db, int32_t n_surf_tab,
                             const double* beta_x, const double* beta_deg, int32_t n_beta, double* out_db, int32_t* nb,
                             int32_t* ns, void* stream);

/* ---- Caustic index and coherent ray-tube pressure: pgr_fan_caustic_index, pgr_caustic_index_device,
 * pgr_fan_pressure_w, pgr_pressure_device_w.  Part of this ABI, stated in a file of their own beside this one. ---- */
#include "pgr_coherent.h"

/* ---- Received time series of a Gaussian pulse from ray-tube arrivals: pgr_signal_device.  Part of
 * this ABI, stated in a file of its own beside this one. ---- */
#include "pgr_signal.h"

/* ---- Transfer function of the arrivals over a frequency band: pgr_spectrum_device.  Part of this
 * ABI, stated in a file of its own beside this one. ---- */
#include "pgr_spectrum.h"

/* ---- The coherent sums with a lag per arrival, the bottom's complex reflection coefficient:
 * pgr_fan_pressure_phi, pgr_pressure_device_phi, pgr_signal_device_phi, pgr_spectrum_device_phi.  Part of this ABI, stated in
 * a file of its own beside this one. ---- */
#include "pgr_reflection.h"

/* ---- Coherent Gaussian-beam pressure with wavefront curvature: pgr_fan_beam_pressure_w,
 * pgr_beam_pressure_device_w.  Part of this ABI, stated in a file of its own beside this one. ---- */
#include "pgr_beam_coherent.h"

/* ---- Gaussian-beam arrivals, the terms of the coherent beam sum listed per receiver:
 * pgr_fan_beam_arrival_counts_w, pgr_fan_beam_arrivals_w, pgr_beam_arrival_counts_device_w, pgr_beam_arrivals_device_w.  Part
 * of this ABI, stated in a file of its own beside this one. ---- */
#include "pgr_beam_arrivals.h"

/* ---- Vertical-array beamforming, the time-angle response from the elements' arrival lists:
 * pgr_array_response_device.  Part of this ABI, stated in a file of its own beside this one. ---- */
#include "pgr_array.h"

/* ---- Matched-field processing, the Bartlett ambiguity surface from the elements' arrival lists:
 * pgr_matched_field_device.  Part of this ABI, stated in a file of its own beside this one (named before pgr_band.h, which
 * stays the last). ---- */
#include "pgr_match.h"

/* ---- Band-averaged power, the transfer function's squared magnitude summed over a band:
 * pgr_band_power_device.  Part of this ABI, stated in a file of its own beside this one. ---- */
#include "pgr_band.h"

/* What this build of the library is: whether the instruction-layout pass of the build was applied
 * ("relaid: 502 -> 31 straddles ..." or "plain hipcc") and which arithmetic variant was compiled.
 * bench.py puts it into its JSON line so that a measured number names the binary it came from. */
const char* pgr_build_info(void);

/* Message for the last error on the calling thread. */
const char* pgr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PGR_H */
