"""pygenray_amd -- MI355X-native drop-in for pygenray's ray-fan hot path.

Same public surface as ``pygenray`` (REF/__init__.py:5-10 star-exports): ``OceanEnvironment2D``,
``shoot_rays``, ``shoot_ray``, ``find_eigenrays``, ``Ray``, ``RayFan``, ``EigenRays``, ``munk_ssp``,
``eflat`` ... -- with the per-ray integration running in hand-written HIP on gfx950 behind the
C ABI of ``include/pgr.h``.  There is no CPU fallback: importing works anywhere, shooting rays
needs ``libpgr_hip.so`` and a GPU.
"""
from .xr_lite import DataArray
from .environment import OceanEnvironment2D, munk_ssp, eflat, eflatinv, flat_earth_c
from .ray_objects import Ray, RayFan, BounceLog, TimeFront, EigenRays
from .launch_rays import shoot_rays, shoot_ray, _unpack_envi
from .eigenrays import find_eigenrays
from .transmission import transmission_loss, beam_transmission_loss
from .arrivals import arrivals, Arrivals
from .sensitivity import travel_time_kernel
from .absorption import thorp_absorption, path_length, path_loss
from .boundary import boundary_loss
from .coherent import (caustic_index, pressure_field, coherent_transmission_loss, beam_pressure_field,
                       coherent_beam_transmission_loss)
from .signal import received_signal, pulse_sigma
from .spectrum import transfer_function, received_waveform
from .beam_arrivals import (beam_arrivals, BeamArrivals, beam_received_signal, beam_transfer_function,
                            beam_received_waveform)
from .array import steering_delays, array_response, beam_array_response
from .band import band_intensity, band_transmission_loss, beam_band_intensity, beam_band_transmission_loss
from .match import matched_field, beam_matched_field
from .reflection import BottomReflection, fluid_halfspace
from .host_physics import (derivsrd, bottom_bounce, surface_bounce, ray_bounding_box_event,
                           ray_angle, bilinear_interp, linear_interp, vertical_ray)
from . import _lib

# "reference" (default: bit-identical to the CPU oracle) or "contracted" (PGR_ARITH=contracted at import: FMA contraction
# allowed, ~10 % faster, no bit-parity claim) -- see pygenray_amd/_lib.py
ARITHMETIC = _lib.ARITH

__all__ = ["OceanEnvironment2D", "munk_ssp", "eflat", "eflatinv", "flat_earth_c", "DataArray", "Ray", "RayFan", "TimeFront",
           "EigenRays", "shoot_rays", "shoot_ray", "find_eigenrays", "transmission_loss", "beam_transmission_loss", "arrivals", "Arrivals",
           "travel_time_kernel", "thorp_absorption", "path_length", "path_loss", "boundary_loss", "BounceLog", "caustic_index", "pressure_field",
           "coherent_transmission_loss", "beam_pressure_field", "coherent_beam_transmission_loss", "received_signal", "pulse_sigma", "transfer_function", "received_waveform", "beam_arrivals",
           "BeamArrivals", "beam_received_signal", "beam_transfer_function", "beam_received_waveform", "steering_delays",
           "array_response", "beam_array_response", "band_intensity", "band_transmission_loss", "beam_band_intensity",
           "beam_band_transmission_loss", "matched_field", "beam_matched_field", "BottomReflection",
           "fluid_halfspace", "derivsrd", "bottom_bounce",
           "surface_bounce", "ray_bounding_box_event", "ray_angle", "bilinear_interp",
           "linear_interp", "vertical_ray"]
