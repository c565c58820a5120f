#!/usr/bin/env python3
"""Elastic constants and equation of state of fcc Cu on the MI355X engine.

    python examples/elastic.py

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  The 32-atom cubic cell is relaxed with its cell first (Relaxer); the 4-atom conventional
cell at the relaxed lattice constant then goes through Elasticity (24 strained copies and the unstrained one, one engine batch) and
EquationOfState.  Prints C_ij, the moduli, the stability verdict and V0, B0, B0'.

This model's energy is not continuous where a neighbour shell crosses its 5 A cutoff, and the fourth fcc shell sits at 4.95 A: the
equation of state samples +-0.75 % linear strain, inside which none crosses (the default +-5 % would fit a curve with a step in it)."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.elasticity import Elasticity, EquationOfState  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.relax import Relaxer  # noqa: E402

model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
a = 3.5
(rel,) = Relaxer(model, relax_cell=True).relax([np.eye(3) * 2 * a], [(grid + base[None]).reshape(-1, 3) * a], [np.full(32, 29)], fmax=1e-3)
a0 = float(np.trace(rel["lattice"])) / 6
print(f"relaxed: a0 = {a0:.4f} A  ({rel['n_steps']} FIRE steps, converged={rel['converged']})")
cell = ([np.eye(3) * a0], [base * a0], [np.full(4, 29)])

t0 = time.perf_counter()
(el,) = Elasticity(model).run(*cell)
print(f"elastic constants (25 copies, ions relaxed in every copy: {el.n_unconverged} unconverged): {time.perf_counter() - t0:.2f} s")
print("C (GPa), Voigt order xx yy zz yz zx xy:")
for row in el.C_gpa:
    print("  " + " ".join(f"{x:8.2f}" for x in row))
print(f"asymmetry {el.asymmetry * 160.21766208:.1e} GPa  fit residual {el.fit_residual * 160.21766208:.2f} GPa  "
      f"residual stress {np.abs(el.residual_stress_gpa).max():.3f} GPa")
print(f"K  Voigt / Reuss / Hill  {el.k_voigt_gpa:.2f} / {el.k_reuss_gpa:.2f} / {el.k_hill_gpa:.2f} GPa")
print(f"G  Voigt / Reuss / Hill  {el.g_voigt_gpa:.2f} / {el.g_reuss_gpa:.2f} / {el.g_hill_gpa:.2f} GPa")
print(f"E {el.youngs_modulus_gpa:.2f} GPa  nu {el.poisson_ratio:.4f}  universal anisotropy {el.universal_anisotropy:.4f}")
print("eigenvalues of C (GPa): " + " ".join(f"{x:.2f}" for x in el.eigenvalues_gpa) + f"  stable={el.stable}")

t0 = time.perf_counter()
(eos,) = EquationOfState(model, strains=np.linspace(-0.0075, 0.0075, 11)).run(*cell)
print(f"equation of state (11 volumes): {time.perf_counter() - t0:.2f} s")
print(f"V0 {eos.v0:.4f} A^3 (a = {eos.v0 ** (1 / 3):.4f} A)  E0 {eos.e0:.5f} eV  B0 {eos.b0_gpa:.2f} GPa  B0' {eos.b0_prime:.2f}  "
      f"rms residual {eos.rms_residual:.1e} eV  error={eos.error}")
print(f"(C11 + 2 C12) / 3 = {(el.C_gpa[0, 0] + 2 * el.C_gpa[0, 1]) / 3:.2f} GPa")
