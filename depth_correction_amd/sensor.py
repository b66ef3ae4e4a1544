"""Gaussian-beam sensor model (the reference's sensor.py, restated) and the footprint pattern of the finite-beam renderer.

Rayleigh range z_R = pi w0^2 n / lambda, beam radius w(z) = w0 M^2 sqrt(1 + (z / z_R)^2), beam propagation factor
M^2 = theta pi w0 / lambda.  The reference's spelling ``rayleight_length`` is kept: it is its public name.

The renderer (render.BeamModel, ops.raycast_beams) does not use ``beam_radius``: with M^2 derived from the divergence, w(0) = w0 M^2
is 13.9 cm for a 2.5 mm waist.  It takes the two raw fields of a Sensor instead -- the 1/e^2 aperture radius r0 = waist_radius and the
1/e^2 half divergence theta = divergence -- and a footprint radius r0 + z tan(theta) at the axial depth z (DESIGN "Finite-beam
rendering").
"""
from __future__ import annotations

import math

import numpy as np
import torch

__all__ = [
    'beam_radius',
    'Medium',
    'Media',
    'rayleight_length',
    'Sensor',
    'Sensors',
    'beam_propagation_factor',
    'beam_pattern',
]


class Medium(object):
    def __init__(self, refractive_index=None):
        self.refractive_index = refractive_index


class Media(object):
    AIR = Medium(refractive_index=1.000293)
    VACUUM = Medium(refractive_index=1.0)


def _tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def rayleight_length(waist_radius, wavelength, n=Media.AIR.refractive_index):
    """Rayleigh range [m] of a beam with the waist radius ``waist_radius`` [m] and the wavelength ``wavelength`` [m] in a medium of
    refractive index ``n`` (1.000293 for air, the default; 1.0 for vacuum)."""
    return torch.pi * _tensor(waist_radius) ** 2 * n / wavelength


def beam_radius(z, waist_radius, wavelength, m2, n=Media.AIR.refractive_index):
    """Beam radius [m] at the depth ``z`` [m]; ``m2`` is the beam propagation factor M^2 (1.0 for an ideal Gaussian beam)."""
    z, waist_radius = _tensor(z), _tensor(waist_radius)
    return waist_radius * m2 * torch.sqrt(1.0 + (z / rayleight_length(waist_radius, wavelength=wavelength, n=n)) ** 2)


def beam_propagation_factor(divergence, waist_radius, wavelength):
    """M^2 of a beam with the half divergence ``divergence`` [rad]."""
    return divergence * torch.pi * waist_radius / wavelength


class Sensor(object):
    """A lidar's beam: wavelength [m], waist radius [m] and either the half divergence [rad] (M^2 is derived from it) or M^2."""

    def __init__(self, name=None, wavelength=None, waist_radius=None, divergence=None, m2=1.0):
        self.name = name
        self.wavelength = wavelength
        self.waist_radius = waist_radius
        self.divergence = divergence
        self.m2 = self.beam_propagation_factor() if divergence is not None else m2

    def rayleight_length(self, n=Media.AIR.refractive_index):
        return rayleight_length(self.waist_radius, n=n, wavelength=self.wavelength)

    def beam_radius(self, z, n=Media.AIR.refractive_index):
        return beam_radius(z, waist_radius=self.waist_radius, n=n, wavelength=self.wavelength, m2=self.m2)

    def beam_propagation_factor(self):
        return beam_propagation_factor(self.divergence, self.waist_radius, self.wavelength)

    def __str__(self):
        return self.name


class Sensors(object):
    # the reference gives both sensors the Ouster's waist radius and divergence
    HOKUYO = Sensor(name='Hokuyo UTM-30LX', wavelength=905e-9, waist_radius=5e-3 / 2, divergence=np.radians(0.35))
    OUSTER = Sensor(name='Ouster OS0', wavelength=865e-9, waist_radius=5e-3 / 2, divergence=np.radians(0.35))


def beam_pattern(n_samples, rho_max=1.5):
    """Footprint samples of a Gaussian beam, float64 [n_samples, 3] with rows (px, py, weight) in units of the 1/e^2 radius: equal-power
    sampling of the Gaussian truncated at ``rho_max`` on a Vogel spiral.  For j = 0 .. S-1: u_j = j / S,
    rho_j = sqrt(-1/2 log1p(-u_j (1 - exp(-2 rho_max^2)))), phi_j = j pi (3 - sqrt 5), (px, py) = rho_j (cos phi_j, sin phi_j),
    weight 1.  Sample 0 is the beam axis."""
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
        raise ValueError('n_samples must be an int >= 1, got %r' % (n_samples,))
    rho_max = float(rho_max)
    if not (math.isfinite(rho_max) and rho_max > 0.0):
        raise ValueError('rho_max must be positive and finite, got %r' % (rho_max,))
    j = np.arange(int(n_samples), dtype=np.float64)
    u = j / float(n_samples)
    rho = np.sqrt(-0.5 * np.log1p(-u * (1.0 - math.exp(-2.0 * rho_max ** 2))))
    phi = j * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), np.ones_like(rho)], axis=1)
