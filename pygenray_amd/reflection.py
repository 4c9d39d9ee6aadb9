"""The bottom's complex plane-wave reflection coefficient for the coherent products: ``BottomReflection``, a table of |R| and
arg R against grazing angle, and ``fluid_halfspace``, the Rayleigh coefficient of a fluid sediment as such a table (DESIGN.md,
"Complex bottom reflection").

Host only: the table is built and checked here and handed to the products through their ``bottom_loss=`` keyword.  Its
magnitude becomes the boundary loss every product already takes; its phase becomes a lag in cycles that the bounce post-pass
(csrc/pgr_bounce.h) accumulates per ray and the coherent sums (csrc/pgr_reflect.h) turn every arrival back by.
"""
import math

import numpy as np

# attenuation in dB per wavelength -> the imaginary part of the index of refraction: 1 / (40 pi log10 e)
_DB_PER_WAVELENGTH = 1.0 / (40.0 * math.pi * math.log10(math.e))
INTROMISSION = 1e-6                   # fluid_halfspace refuses a table with |R| below this at a node


def _sequence(v, name):
    a = np.array(v, dtype=float)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a 1-D sequence")
    return a


class BottomReflection:
    """A tabulated complex plane-wave reflection coefficient of the bottom: ``magnitude`` |R| in (0, 1] and ``phase_deg`` =
    arg R in degrees on the nodes ``grazing_deg`` (degrees, finite, strictly ascending) -- three 1-D sequences of equal
    length >= 1; linear between the nodes, held at the end values outside them (magnitude: linear in dB).

    The convention is ``pressure_field``'s: a path of delay T carries exp(+2 pi i f T), so ``phase_deg`` is arg R for the time
    dependence e^{-i w t}; total reflection from a fast bottom has a negative phase.  ``phase_deg`` is finite and given
    UNWRAPPED: it is interpolated linearly, so a 360 degree jump between two nodes is the caller's error.

    Pass it as ``bottom_loss=``: ``transmission_loss``, ``beam_transmission_loss``, ``arrivals`` and ``boundary_loss`` use
    its magnitude (``.loss``); ``pressure_field``, ``coherent_transmission_loss``, ``received_signal``, ``transfer_function``
    and ``received_waveform`` also its phase (``.lag``).  Two views:

    - ``loss``: ``(grazing_deg, max(0, -20 log10 magnitude))``, the pair ``bottom_loss=`` takes as dB per bounce;
    - ``lag``: ``(grazing_deg, n - phase_deg / 360)`` in cycles, n the smallest integer >= 0 that makes every node >= 0
      (whole cycles change nothing; the accumulating entry takes no negative table values).

    ``ValueError`` for everything else."""

    def __init__(self, grazing_deg, magnitude, phase_deg):
        g, m, p = _sequence(grazing_deg, "grazing_deg"), _sequence(magnitude, "magnitude"), _sequence(phase_deg, "phase_deg")
        if not (len(g) == len(m) == len(p)) or len(g) == 0:
            raise ValueError("grazing_deg, magnitude and phase_deg must be three 1-D sequences of equal, non-zero length")
        if not np.all(np.isfinite(g)) or not np.all(np.diff(g) > 0):
            raise ValueError("grazing_deg must be finite and strictly ascending")
        if not np.all((m > 0) & (m <= 1)):                       # (False for a NaN)
            raise ValueError("magnitude must lie in (0, 1]")
        if not np.all(np.isfinite(p)):
            raise ValueError("phase_deg must be finite (and unwrapped)")
        for a in (g, m, p):
            a.flags.writeable = False
        self.grazing_deg, self.magnitude, self.phase_deg = g, m, p

    def __len__(self):
        return len(self.grazing_deg)

    @property
    def loss(self):
        db = np.maximum(0.0, -20.0 * np.log10(self.magnitude)) + 0.0           # (+ 0.0: no negative zero)
        return self.grazing_deg.copy(), db

    @property
    def lag(self):
        v = -self.phase_deg / 360.0
        n = max(0, int(math.ceil(-float(v.min()))))
        while np.any(n + v < 0.0):                               # (n + v rounds: one more cycle when it rounds below zero)
            n += 1
        return self.grazing_deg.copy(), n + v

    def __call__(self, grazing_deg):
        """R at the grazing angles given (degrees): the table's own interpolation, |R| linear in dB and arg R linear"""
        q = np.asarray(grazing_deg, dtype=float)
        db = np.interp(q, self.grazing_deg, self.loss[1])
        ph = np.interp(q, self.grazing_deg, self.phase_deg)
        return 10.0 ** (-db / 20.0) * np.exp(1j * np.radians(ph))

    def __repr__(self):
        return (f"BottomReflection({len(self)} nodes, {self.grazing_deg[0]:g} ... {self.grazing_deg[-1]:g} degrees, |R| "
                f"{self.magnitude.min():.3g} ... {self.magnitude.max():.3g})")


def _positive(v, name):
    x = float(v)
    if not (math.isfinite(x) and x > 0):
        raise ValueError(f"{name} must be finite and > 0")
    return x


def fluid_halfspace(sound_speed, density, attenuation=0.0, water_sound_speed=1500.0, water_density=1000.0, step_deg=0.05):
    """The Rayleigh reflection coefficient of a homogeneous fluid half-space -- ``sound_speed`` (m/s), ``density`` (kg/m^3),
    ``attenuation`` (dB per wavelength, >= 0) -- under water of ``water_sound_speed`` and ``water_density``, tabulated on the
    grazing angles 0, ``step_deg``, ... 90 degrees -> ``BottomReflection``:

        m = density / water_density
        n = (water_sound_speed / sound_speed) (1 + i attenuation / (40 pi log10 e))
        R(theta) = (m sin(theta) - Q) / (m sin(theta) + Q),   Q = sqrt(n^2 - cos(theta)^2),  Im Q >= 0

    in ``pressure_field``'s convention (total reflection has a negative phase).  The lag -arg R / 2 pi is taken as
    -(arg(numerator) - arg(denominator)) / 2 pi with arg(numerator) in [-pi, 0], which makes it >= 0 and continuous in
    theta; a lossless bottom's |R| = 1 + 4e-16 below the critical angle is held at 1 (0 dB).  R does not depend on frequency
    (the attenuation is per wavelength), so ``transfer_function`` applies the one table across its band.

    Two limits.  The water sound speed is the table's, not the environment's at each bounce.  For ``attenuation=0`` the
    square-root kink of R at the critical angle is not linear: the table misses R by up to 0.03 within 0.5 degrees of it at
    the default step (6e-5 elsewhere); with 0.5 dB per wavelength the miss is 1.9e-5 everywhere.

    ``ValueError`` for parameters that are not finite and positive (``attenuation``: >= 0), a ``step_deg`` outside (0, 90],
    and for a bottom with an angle of intromission -- a node where |R| < 1e-6, whose phase is undefined: the angle is
    named."""
    cb, rb = _positive(sound_speed, "sound_speed"), _positive(density, "density")
    cw, rw = _positive(water_sound_speed, "water_sound_speed"), _positive(water_density, "water_density")
    a = float(attenuation)
    if not (math.isfinite(a) and a >= 0):
        raise ValueError("attenuation must be finite and >= 0 dB per wavelength")
    step = float(step_deg)
    if not (math.isfinite(step) and 0 < step <= 90):
        raise ValueError("step_deg must lie in (0, 90] degrees")
    count = int(math.ceil(90.0 / step - 1e-9))
    theta = np.minimum(np.arange(count + 1) * step, 90.0)
    theta[-1] = 90.0
    if not np.all(np.diff(theta) > 0):
        raise ValueError("step_deg is too small for the nodes to ascend")
    rad = np.radians(theta)
    ms = (rb / rw) * np.sin(rad)
    n = (cw / cb) * complex(1.0, a * _DB_PER_WAVELENGTH)
    Q = np.sqrt(n * n - np.cos(rad) ** 2 + 0j)
    Q = np.where(Q.imag < 0, -Q, Q)
    num, den = ms - Q, ms + Q
    with np.errstate(invalid="ignore", divide="ignore"):
        mag = np.abs(num) / np.abs(den)                          # (0 / 0 for a bottom that is the water: refused below)
    low = np.flatnonzero(~(mag >= INTROMISSION))
    if len(low):
        raise ValueError(f"the bottom has an angle of intromission: |R| = {mag[low[0]]:.3g} at {theta[low[0]]:g} degrees "
                         f"grazing, where the phase of R is undefined (below {INTROMISSION:g})")
    lag = -(np.arctan2(-np.abs(num.imag), num.real) - np.arctan2(den.imag, den.real)) / (2.0 * np.pi)
    return BottomReflection(theta, np.minimum(mag, 1.0), -360.0 * lag)


__all__ = ["BottomReflection", "fluid_halfspace"]
