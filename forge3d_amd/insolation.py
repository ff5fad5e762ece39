"""Sun tracks and clear-sky weights for ``TerrainSession.irradiation`` / ``insolation`` (solar-exposure maps).

``sun_track`` samples one civil day through the NREL ephemeris of ``geo.solar_position``; ``clear_sky`` turns the track's
elevations into beam and diffuse irradiances with two textbook formulas.  Both are host-side float64 arithmetic over a few
dozen sun positions; the per-sample work -- incidence on the local slope, the shadow rays -- is the session's
(``f3d_session_irradiation``).  Measured irradiances go in instead of ``clear_sky`` wherever they exist.
"""
from __future__ import annotations

import numpy as np

from . import geo


def sun_track(date, lat: float, lon: float, *, step_minutes: float = 30, tz_offset_hours: float = 0.0, elev_m: float = 0.0, **spa) -> dict:
    """The sun over the civil day ``date`` (``(year, month, day)`` or a ``datetime.date``) at ``lat`` / ``lon`` (degrees), one
    position per step of ``step_minutes``: the step MIDPOINTS ``(k + 1/2) step`` after local midnight, each through
    ``geo.solar_position`` (``tz_offset_hours``, ``elev_m`` and ``**spa`` -- ``delta_t_seconds``, ``pressure_mbar``,
    ``temperature_c`` -- are its arguments).  Only steps whose APPARENT elevation is above 0 are kept.  Returns a dict of

    * ``directions``  float32 (K, 3): toward the sun, ``(sin az cos el, sin el, -cos az cos el)`` from the azimuth and the apparent
      elevation -- the session's sun convention (azimuth 0 is north, -z; 90 east, +x; y up);
    * ``elevation_deg``  float64 (K,): the apparent elevations;
    * ``hours``  float64 (K,): the length of each step in hours (the weight of a position is irradiance x hours);
    * ``utc``  the K civil tuples ``(year, month, day, hour, minute, second)`` handed to ``solar_position``.
    """
    year, month, day = (date.year, date.month, date.day) if hasattr(date, "year") else (int(v) for v in date)
    step = float(step_minutes)
    if not (step > 0.0 and step <= 1440.0):
        raise ValueError(f"step_minutes must be in (0, 1440], got {step_minutes}")
    steps = int(np.ceil(1440.0 / step - 1e-9))
    directions, elevations, hours, stamps = [], [], [], []
    for k in range(steps):
        begin, end = k * step, min((k + 1) * step, 1440.0)
        seconds = 0.5 * (begin + end) * 60.0
        hour, rest = divmod(seconds, 3600.0)
        minute, second = divmod(rest, 60.0)
        stamp = (year, month, day, int(hour), int(minute), float(second))
        sun = geo.solar_position(stamp, lat, lon, elev_m, tz_offset_hours=tz_offset_hours, **spa)
        el = float(sun["apparent_elevation_deg"])
        if not el > 0.0:
            continue
        az_r, el_r = np.radians(sun["azimuth_deg"]), np.radians(el)
        directions.append((np.sin(az_r) * np.cos(el_r), np.sin(el_r), -np.cos(az_r) * np.cos(el_r)))
        elevations.append(el)
        hours.append((end - begin) / 60.0)
        stamps.append(stamp)
    return {"directions": np.asarray(directions, np.float64).reshape(-1, 3).astype(np.float32),
            "elevation_deg": np.asarray(elevations, np.float64), "hours": np.asarray(hours, np.float64), "utc": stamps}


def clear_sky(elevation_deg, altitude_m: float = 0.0):
    """Clear-sky irradiances ``(dni, dhi)`` in W/m^2 (float64, the shape of ``elevation_deg``) for apparent sun elevations in
    degrees at ``altitude_m`` above sea level; both are 0 at ``el <= 0``.

    * air mass, Kasten-Young (1989): ``AM = 1 / (sin el + 0.50572 (el + 6.07995)^-1.6364)``;
    * beam, Meinel / Laue: ``dni = 1353 ((1 - 0.14 a) 0.7^(AM^0.678) + 0.14 a)``, ``a`` the altitude in km;
    * diffuse: ``dhi = 0.1 dni``.

    The diffuse tenth is a RULE OF THUMB for a clear day, and the whole model knows nothing of turbidity, water vapour or
    cloud: where irradiances were measured (or come from a climate file), hand those to ``TerrainSession.insolation`` /
    ``irradiation`` as the weights instead."""
    el = np.asarray(elevation_deg, np.float64)
    up = el > 0.0
    safe = np.where(up, el, 90.0)
    air_mass = 1.0 / (np.sin(np.radians(safe)) + 0.50572 * (safe + 6.07995) ** -1.6364)
    a = float(altitude_m) / 1000.0
    dni = np.where(up, 1353.0 * ((1.0 - 0.14 * a) * 0.7 ** (air_mass ** 0.678) + 0.14 * a), 0.0)
    return dni, 0.1 * dni


__all__ = ["sun_track", "clear_sky"]
