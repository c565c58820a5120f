#!/usr/bin/env python3
"""Anharmonic Helmholtz free energy of the 32-atom Cu cell under the LJ-fitted model by thermodynamic integration to an Einstein
crystal (torch_m3gnet.free_energy), at a few temperatures, beside the harmonic free energy of torch_m3gnet.phonons plus the static
lattice energy.  Both are classical and of the same cell here (the harmonic column is the classical limit kB T sum ln(hbar w / kB T)
over the 3 n - 3 modes the cell holds, with the centre-of-mass terms of `einstein_free_energy`), so what separates them is
anharmonicity.

    python examples/free_energy.py [switch steps] [replicas]

The lattice constant (3.35 A) keeps every neighbour shell a quarter of an angstrom from the model's two-body cutoff: the model's
energy steps where a pair crosses it, and thermodynamic integration needs an energy that is the integral of its forces
(DESIGN.md section 7j)."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "torch-m3gnet_amd"))
from torch_m3gnet.data import MaterialGraphKey as K  # noqa: E402
from torch_m3gnet.data.md import VerletGraph  # noqa: E402
from torch_m3gnet.free_energy import FreeEnergy  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.path_integral import HBAR  # noqa: E402
from torch_m3gnet.phonons import Phonons  # noqa: E402

switch_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
replicas = int(sys.argv[2]) if len(sys.argv) > 2 else 4
KB, KAPPA, A = 8.617333262e-5, 9.648533215665e-3, 3.35
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")

base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
pos, lat = (grid + base[None]).reshape(-1, 3) * A, np.eye(3) * 2 * A
z = np.full(32, 29)

# the static lattice energy and the harmonic frequencies of the same cell (Gamma of the 32-atom cell: the modes the cell holds)
vg = VerletGraph([lat], [z], 5.0, 4.0, skin=0.5, device="cuda")
e0 = float(vg.step(model, torch.tensor(pos, device="cuda"))[K.TOTAL_ENERGY][0])
(res,) = Phonons(model).run([lat], [pos], [z], (1, 1, 1))
freq = res.frequencies(np.zeros((1, 3)))[0]      # THz
omega = 2.0 * np.pi * freq[3:] * 1e-3            # rad/fs, without the three acoustic zeros
print(f"static energy {e0:.4f} eV; {len(omega)} modes of the cell, {freq[3]:.2f} .. {freq.max():.2f} THz")
print(f"{'T (K)':>6} {'F harmonic':>12} {'F integrated':>14} {'+-':>7} {'k (eV/A^2)':>11} {'dissipation':>12}")
mass, volume = float(res.masses[0]), abs(np.linalg.det(lat))
for t in (50.0, 100.0, 200.0):
    kt = KB * t
    # the classical harmonic crystal in the convention of einstein_free_energy: the 3 n - 3 modes with the centre of mass held at a
    # point (delta(R_cm) = n^(3/2) delta(Q_cm) in the orthonormal mode coordinates), all 3 n momenta, and the crystal free to sit
    # anywhere in a primitive cell: kT ln[(n_cells / V) Lambda^3 / n^(3/2)], Lambda the thermal wavelength of one atom
    wavelength2 = 2.0 * np.pi * HBAR ** 2 * KAPPA / (mass * kt)
    f_harm = e0 + kt * np.log(HBAR * omega / kt).sum() + kt * np.log(len(z) / volume * wavelength2 ** 1.5 / len(z) ** 1.5)
    fe = FreeEnergy(model, t, "msd", timestep=2.0, replicas=replicas, seed=0)
    (out,) = fe.switch([lat], [pos], [z], equilibration=500, switch_steps=switch_steps)
    print(f"{t:6.0f} {f_harm:12.4f} {out['free_energy']:14.4f} {out['free_energy_error']:7.4f} {out['spring_constants'][0]:11.3f} "
          f"{out['dissipation'].mean():12.4f}")
print("eV per cell, classical nuclei on both sides: what separates the columns is anharmonicity.")
