"""Standard atomic weights (amu) for Z = 1 - 95, the species range of the model (num_types = 95): the IUPAC abridged values (4-5
significant digits).  Elements without a stable isotope (Tc, Pm, Po - Rn, Fr - Ac, Np - Am) take the mass number of their
longest-lived isotope.  These are the default masses of torch_m3gnet.dynamics; a caller may pass per-atom masses instead."""
from __future__ import annotations

import numpy as np

# index Z - 1
ATOMIC_MASSES = np.array([
    1.008, 4.0026, 6.94, 9.0122, 10.81, 12.011, 14.007, 15.999, 18.998, 20.180,                         # H  - Ne
    22.990, 24.305, 26.982, 28.085, 30.974, 32.06, 35.45, 39.95, 39.098, 40.078,                         # Na - Ca
    44.956, 47.867, 50.942, 51.996, 54.938, 55.845, 58.933, 58.693, 63.546, 65.38,                       # Sc - Zn
    69.723, 72.630, 74.922, 78.971, 79.904, 83.798, 85.468, 87.62, 88.906, 91.224,                       # Ga - Zr
    92.906, 95.95, 97.0, 101.07, 102.91, 106.42, 107.87, 112.41, 114.82, 118.71,                         # Nb - Sn
    121.76, 127.60, 126.90, 131.29, 132.91, 137.33, 138.91, 140.12, 140.91, 144.24,                      # Sb - Nd
    145.0, 150.36, 151.96, 157.25, 158.93, 162.50, 164.93, 167.26, 168.93, 173.05,                       # Pm - Yb
    174.97, 178.49, 180.95, 183.84, 186.21, 190.23, 192.22, 195.08, 196.97, 200.59,                      # Lu - Hg
    204.38, 207.2, 208.98, 209.0, 210.0, 222.0, 223.0, 226.0, 227.0, 232.04,                             # Tl - Th
    231.04, 238.03, 237.0, 244.0, 243.0,                                                                 # Pa - Am
])
assert len(ATOMIC_MASSES) == 95


def masses_of(atomic_numbers) -> np.ndarray:
    """Default masses [n] (amu) of atomic numbers in 1..95; anything else raises ValueError."""
    z = np.asarray(atomic_numbers).reshape(-1)
    if z.size and (not np.issubdtype(z.dtype, np.integer) or z.min() < 1 or z.max() > len(ATOMIC_MASSES)):
        raise ValueError(f"atomic numbers must be integers in 1..{len(ATOMIC_MASSES)} (no default mass otherwise)")
    return ATOMIC_MASSES[z.astype(np.int64) - 1].copy()
