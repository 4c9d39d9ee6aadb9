// pgr_hip.hip -- MI355X (gfx950) ray-fan integrator behind the C ABI of include/pgr.h.
//
// One ray per lane (wave64).  Every lane runs SciPy's adaptive Dormand-Prince 5(4)
// controller on the ray equations y = [T, z, p] over range x with the reference's
// bilinear c / dc/dz tables, +-1 step-function events located by brentq-style
// bisection on the quartic dense output, reflection at surface / bottom and the
// reference's nearest-index re-sampling -- restating, on the device,
//   REF/integration_processes.py:26-334   (derivsrd, bilinear/linear interp, events)
//   REF/launch_rays.py:325-484, 593-681    (_shoot_ray_array, _shoot_ray_segment)
//   REF/launch_rays.py:745-784             (_interpolate_ray)
//   SCIPY/rk.py:14-180,377-404,552-574 ; SCIPY/common.py:63-134 ; SCIPY/ivp.py:28-156,654-726
// (REF = /root/reference/src/pygenray, SCIPY = scipy/integrate/_ivp of SciPy 1.15.3).
//
// Layout: the c and dc/dz tables are interleaved node-wise as double2 {c, cp} so one
// 16-byte access fetches both values of a node; for range-independent tables the single
// depth profile (nz x 16 B, 96 KB at nz = 6000) is staged into LDS once per workgroup, next
// to zin and its bucket table when the depth grid is not uniform, and the bathymetry.
// State (x, y, f, h, K1..K7) lives in VGPRs.  No MFMA: there is no contraction here.
//
// Arithmetic that feeds back into the integration is written in the reference's operation
// order and compiled with -ffp-contract=off; divide / sqrt are correctly rounded, the three libm
// calls of the reference (err ** -0.2, arcsin, sin) are evaluated CORRECTLY ROUNDED
// (pgr_crmath.h) and the event locator returns brentq's own root, so the result is bit-identical
// to the CPU oracle in its correctly-rounded-libm mode (oracle/ray_oracle.c, ORC_MATH_CR).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <time.h>
#include <float.h>
#include <string>
#include <vector>
#include <mutex>
#include <thread>
#include <atomic>
#include <initializer_list>
#include <limits>

#include "../../include/pgr.h"
#include "pgr_crmath.h"
#include "pgr_device.h"      // descriptor, arithmetic, look-ups, events, dense output, stage macros
#include "pgr_fan_kernel.h"  // the fan kernel
// the rest of this translation unit, in dependency order (one TU: the instruction-layout pass of the build works on ONE
// device object, and the kernels' order in it is part of what device_code_sha256 names)
#include "pgr_aux_kernels.h"    // wave cost / placement kernels, unit-level test kernels
#include "pgr_host.h"           // error handling, struct pgr_env, buffers, fan buffer layout, pgr_build_info
#include "pgr_env.h"            // environment construction + host-side verification, options, queries
#include "pgr_launch.h"         // wave scheduling, pgr_shoot_fan_device
#include "pgr_transfer.h"       // compaction, pipelined D2H, pgr_shoot_fan
#include "pgr_fan_handle.h"     // pgr_initial_states_device, pgr_fan_*
#include "pgr_eigen_hist.h"     // pgr_eigen_refine*, pgr_arrival_histogram_device
#include "pgr_debug_entry.h"    // pgr_debug_math / pgr_debug_step / pgr_eval_points
#include "pgr_tl.h"             // ray-tube intensity / transmission loss: pgr_fan_intensity, pgr_intensity_device
#include "pgr_arrivals.h"       // ray-tube arrivals at receiver depths: pgr_fan_arrival_counts, pgr_fan_arrivals, ..._device
#include "pgr_beams.h"          // Gaussian-beam intensity: pgr_fan_beam_intensity, pgr_beam_intensity_device
#include "pgr_sens.h"           // travel-time sensitivity kernels: pgr_fan_travel_time_kernel, pgr_travel_time_kernel_device
#include "pgr_front.h"          // time fronts and turning-point counts: pgr_fan_time_front, pgr_time_front_device
#include "pgr_path.h"           // path integrals, absorption weights: pgr_fan_path_integral, pgr_path_integral_device
#include "pgr_bounce.h"         // boundary reflection loss from a fan's bounce log: pgr_fan_boundary_loss, pgr_boundary_loss_device
#include "pgr_phase.h"          // caustic index of the tubes and their coherent sum: pgr_fan_caustic_index, pgr_fan_pressure_w, ..._device
#include "pgr_beam_phase.h"     // coherent Gaussian-beam pressure with wavefront curvature: pgr_fan_beam_pressure_w, pgr_beam_pressure_device_w
#include "pgr_beam_arrivals.h"  // the terms of that sum listed as arrivals: pgr_fan_beam_arrival_counts_w, pgr_fan_beam_arrivals_w, ..._device_w
#include "pgr_signal.h"         // received time series of a Gaussian pulse from the arrivals: pgr_signal_device
#include "pgr_reflect.h"        // the coherent sums with a lag per arrival (complex bottom reflection): pgr_fan_pressure_phi, pgr_signal_device_phi, ...
#include "pgr_array.h"          // vertical-array beamforming, delay-and-sum over the arrivals (pgr_signal.h's helpers): pgr_array_response_device
#include "pgr_band.h"           // band-averaged power, pgr_spectrum.h's sum reduced over frequency (it includes pgr_spectrum.h first): pgr_band_power_device
#include "pgr_match.h"          // matched-field processing, that sum folded with the array's data over elements and frequency: pgr_matched_field_device
#include "pgr_spectrum.h"       // transfer function of the arrivals over a frequency band: pgr_spectrum_device
