"""The low-level binding API of pygenray_amd._lib that tests and scripts call: every ``FanHandle`` product method and every
``*_device`` function keeps its parameter names, their order and their defaults (no GPU, no library needed)."""
import inspect

from pygenray_amd import _lib

HANDLE = {
    "boundary_loss": "(self, tables, out_ptr, nb_ptr=0, ns_ptr=0, stream=0)",
    "intensity": "(self, p0_ptr, depths_ptr, n_depths, out_ptr, stream=0, weights=0)",
    "path_integral": "(self, a_depths, alpha, out_ptr, stream=0)",
    "beam_intensity": "(self, p0_ptr, bottom_ptr, depths_ptr, n_depths, min_width, out_ptr, stream=0, weights=0)",
    "arrival_counts": "(self, p0_ptr, depths_ptr, n_depths, cols, counts_ptr, stream=0)",
    "arrivals": "(self, p0_ptr, depths_ptr, n_depths, cols, offsets_ptr, n_arrivals, tube_ptr, w_ptr, t_ptr, p_ptr, i_ptr, stream=0, weights=0)",
    "travel_time_kernel": "(self, ranges_ptr, n_ranges, depths_ptr, n_depths, column, out_ptr, stream=0)",
    "time_front": "(self, cols, t_ptr, z_ptr, p_ptr, turns_ptr, stream=0)",
    "caustic_index": "(self, nb_ptr, ns_ptr, kappa_ptr, stream=0)",
    "pressure": "(self, p0_ptr, q_ptr, frequency, depths_ptr, n_depths, re_ptr, im_ptr, stream=0, weights=0)",
    "pressure_phi": "(self, p0_ptr, q_ptr, phi_ptr, frequency, depths_ptr, n_depths, re_ptr, im_ptr, stream=0, weights=0)",
    "beam_pressure": "(self, p0_ptr, q_ptr, frequency, bottom_ptr, depths_ptr, n_depths, min_width, curvature, re_ptr, im_ptr, stream=0, weights=0)",
    "beam_arrival_counts": "(self, p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, counts_ptr, stream=0, weights=0)",
    "beam_arrivals": "(self, p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, curvature, offsets_ptr, n_arrivals, tube_ptr, image_ptr, time_ptr, amp_ptr, qa_ptr, stream=0, weights=0)",
}
BUFFER = {
    "initial_states_device": "(device, ang_ptr, n, source_depth, c_source, y0_ptr, stream=0)",
    "arrival_histogram_device": "(device, t_ptr, t_stride, status_ptr, status_stride, n, t_min, t_max, nbins, counts_ptr, stream=0)",
    "intensity_device": "(env, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, depths_ptr, n_depths, out_ptr, stream=0, weights=0)",
    "beam_intensity_device": "(env, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, bottom_ptr, depths_ptr, n_depths, min_width, out_ptr, stream=0, weights=0)",
    "arrival_counts_device": "(env, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, depths_ptr, n_depths, cols, counts_ptr, stream=0)",
    "arrivals_device": "(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, depths_ptr, n_depths, cols, offsets_ptr, n_arrivals, tube_ptr, w_ptr, t_out_ptr, p_out_ptr, i_ptr, stream=0, weights=0)",
    "travel_time_kernel_device": "(env, t_ptr, z_ptr, n_rays, n_samples, x_ptr, ranges_ptr, n_ranges, depths_ptr, n_depths, column, out_ptr, stream=0)",
    "time_front_device": "(device, t_ptr, z_ptr, p_ptr, n_rays, n_samples, cols, t_out_ptr, z_out_ptr, p_out_ptr, turns_ptr, stream=0)",
    "path_integral_device": "(env, t_ptr, z_ptr, n_rays, n_samples, x_ptr, a_depths, alpha, out_ptr, stream=0)",
    "boundary_loss_device": "(env, bx_ptr, bp_ptr, bk_ptr, n_rays, K, x0, x1, n_samples, tables, out_ptr, nb_ptr=0, ns_ptr=0, stream=0)",
    "absorption_weights_device": "(device, a_ptr, n, w_ptr, stream=0)",
    "caustic_index_device": "(device, z_ptr, n_rays, n_samples, nb_ptr, ns_ptr, kappa_ptr, stream=0)",
    "pressure_device": "(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, frequency, depths_ptr, n_depths, re_ptr, im_ptr, stream=0, weights=0)",
    "pressure_phi_device": "(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, phi_ptr, frequency, depths_ptr, n_depths, re_ptr, im_ptr, stream=0, weights=0)",
    "beam_pressure_device": "(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, frequency, bottom_ptr, depths_ptr, n_depths, min_width, curvature, re_ptr, im_ptr, stream=0, weights=0)",
    "beam_arrival_counts_device": "(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, counts_ptr, stream=0, weights=0)",
    "beam_arrivals_device": "(env, t_ptr, z_ptr, p_ptr, n_rays, n_samples, x_ptr, p0_ptr, q_ptr, bottom_ptr, depths_ptr, n_depths, min_width, cols, curvature, offsets_ptr, n_arrivals, tube_ptr, image_ptr, time_ptr, amp_ptr, qa_ptr, stream=0, weights=0)",
    "signal_device": "(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, tstart_ptr, frequency, inv_sigma, dt, n_times, re_ptr, im_ptr, stream=0)",
    "signal_phi_device": "(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi_ptr, tstart_ptr, frequency, inv_sigma, dt, n_times, re_ptr, im_ptr, stream=0)",
    "spectrum_device": "(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, l_ptr, tred_ptr, freq, alpha, re_ptr, im_ptr, stream=0)",
    "spectrum_phi_device": "(device, offsets_ptr, n_groups, t_ptr, i_ptr, q_ptr, phi_ptr, l_ptr, tred_ptr, freq, alpha, re_ptr, im_ptr, stream=0)",
}
# the buffer twin of every handle method -> how many parameters name its fan before the product's own begin: (env or
# device, the trajectory rows it reads, n_rays, n_samples[, x]); the bounce log of boundary_loss_device likewise
FAN_PREFIX = {"boundary_loss": 9, "intensity": 6, "path_integral": 6, "beam_intensity": 6, "arrival_counts": 6, "arrivals": 7,
              "travel_time_kernel": 6, "time_front": 6, "caustic_index": 4, "pressure": 7, "pressure_phi": 7, "beam_pressure": 7,
              "beam_arrival_counts": 7, "beam_arrivals": 7}


def test_binding_signatures_are_the_recorded_ones():
    have = {n: str(inspect.signature(f)) for n, f in vars(_lib).items() if n.endswith("_device") and inspect.isfunction(f)}
    assert have == BUFFER
    assert {n: str(inspect.signature(getattr(_lib.FanHandle, n))) for n in HANDLE} == HANDLE
    # ... and HANDLE is every method of FanHandle that has a buffer twin
    assert {n[:-len("_device")] for n in BUFFER if hasattr(_lib.FanHandle, n[:-len("_device")])} == set(HANDLE)


def test_handle_and_buffer_entries_take_the_same_product_arguments():
    """After `self` and after the fan prefix the two entries of a product name the same parameters with the same defaults.
    (Where a buffer entry reads rows t / z / p of its fan AND writes outputs of those names, its outputs are `t_out_ptr` ...
    and the handle's, which has no such rows, `t_ptr` ...: those names are compared without the `_out`.)"""
    assert set(FAN_PREFIX) == set(HANDLE)
    for name, skip in FAN_PREFIX.items():
        handle = list(inspect.signature(getattr(_lib.FanHandle, name)).parameters.values())[1:]
        buffer = list(inspect.signature(getattr(_lib, name + "_device")).parameters.values())[skip:]
        assert [(p.name, p.default) for p in handle] == [(p.name.replace("_out_ptr", "_ptr"), p.default) for p in buffer], name
        prefix = list(inspect.signature(getattr(_lib, name + "_device")).parameters)[:skip]
        assert prefix[0] in ("env", "device") and prefix[-1] in ("n_samples", "x_ptr"), name
