"""The refusals the C entry points of the eleven driver families that do not integrate share (m3g_fire_*, m3g_lbfgs_*, m3g_neb_*,
m3g_ph_*, m3g_el_*, m3g_traj_*, m3g_nma_*, m3g_remd_*, m3g_mc_*, m3g_rnemd_*, m3g_meta_*), pinned exactly: the status and the whole
m3g_last_error() text of a null state, of a state buffer one byte shorter than the family's *_state_bytes says, of the borrowed dynamics
buffer one byte short (the four calls that take one), and of a null result pointer of every *_state_bytes and *_view.  The other
*_cpu.py files match a word of these messages; here the shared host helpers of csrc/m3g_chunks.h are held to the text.

EXPECTED was recorded from the library of the commit before those helpers existed ("One MD run loop under the eight drivers that
integrate"), not from the code under test.  Every entry is here because its size check precedes its first HIP call (read in the
source of all eleven units), so the library answers without a device; the state pointer is a dummy address that is never followed.
The host arrays of the inits are real and valid, at the smallest sizes a family takes: N = 3, S = 1; S = 2 in one ladder for
m3g_remd_*; one unit atom in a 1x1x1 supercell with one q-point for m3g_nma_*.

Left out: m3g_ph_group_velocities (no state buffer).  No other entry point of the eleven families is left out."""
import ctypes as C

import numpy as np

DUMMY, BIG = C.c_void_p(256), 1 << 30
N, S = 3, 1


def _lib():
    from torch_m3gnet import _lib

    return _lib, _lib.load_library()


def _p(a):
    return a.ctypes.data


class Family:
    """One family at its smallest sizes.  `bytes_calls`: entry -> f(result pointer) -> status, the first one the family's *_state_bytes;
    `calls`: entry -> f(state, nbytes, dyn_bytes) -> status; `borrows`: the calls that take a dynamics state as well."""

    def __init__(self, bytes_calls, calls, borrows=()):
        self.bytes_calls, self.calls, self.borrows = bytes_calls, calls, borrows


def _families():
    _l, lib = _lib()
    keep = []   # the host arrays stay alive as long as the closures

    def arr(values, dtype):
        keep.append(np.ascontiguousarray(np.array(values, dtype=dtype)))
        return _p(keep[-1])

    offsets, lattice = arr([0, N], np.int64), arr(np.eye(3) * 5.0, np.float64)
    positions = arr([[0.0, 0.0, 0.0], [1.0, 0.3, 0.2], [0.4, 1.7, 0.9]], np.float64)
    masses, ones8 = arr([63.546] * N, np.float64), arr([1] * N, np.uint8)
    temps, seeds = arr([300.0, 350.0], np.float64), arr([1, 2], np.uint64)
    fam = {}

    fire = _l.M3GFireParams(dt=1.0, maxstep=0.2, dtmax=10.0, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, fmax=0.05, nmin=5, relax_cell=0)
    fam["fire"] = Family(
        {"m3g_fire_state_bytes": lambda r: lib.m3g_fire_state_bytes(N, S, r)},
        {"m3g_fire_init": lambda st, n, d: lib.m3g_fire_init(C.byref(fire), N, S, offsets, DUMMY, None, st, n, None),
         "m3g_fire_step": lambda st, n, d: lib.m3g_fire_step(C.byref(fire), N, S, st, n, DUMMY, None, DUMMY, None, None, 0, None, None),
         "m3g_fire_read": lambda st, n, d: lib.m3g_fire_read(N, S, st, n, *[None] * 7, None)})

    lbfgs = _l.M3GLbfgsParams(maxstep=0.2, damping=1.0, alpha=70.0, fmax=0.05, memory=1, relax_cell=0)
    fam["lbfgs"] = Family(
        {"m3g_lbfgs_state_bytes": lambda r: lib.m3g_lbfgs_state_bytes(N, S, 1, r)},
        {"m3g_lbfgs_init": lambda st, n, d: lib.m3g_lbfgs_init(C.byref(lbfgs), N, S, offsets, DUMMY, None, st, n, None),
         "m3g_lbfgs_step": lambda st, n, d: lib.m3g_lbfgs_step(C.byref(lbfgs), N, S, st, n, DUMMY, None, DUMMY, None, None, 0, None, None),
         "m3g_lbfgs_read": lambda st, n, d: lib.m3g_lbfgs_read(N, S, 1, st, n, *[None] * 4, None)})

    band, k, climb, ends = arr([0, 1], np.int32), arr([1.0], np.float64), arr([0], np.int32), arr([0.0, 0.0], np.float64)
    fam["neb"] = Family(
        {"m3g_neb_state_bytes": lambda r: lib.m3g_neb_state_bytes(N, 1, 1, r)},
        {"m3g_neb_init": lambda st, n, d: lib.m3g_neb_init(N, 1, 1, offsets, band, k, climb, DUMMY, ends, st, n, None),
         "m3g_neb_forces": lambda st, n, d: lib.m3g_neb_forces(N, 1, 1, st, n, DUMMY, DUMMY, DUMMY, DUMMY, None, None)})

    ph = _l.M3GPhSizes(n_structs=1, n_unit_atoms=N, n_super_atoms=N, n_pairs=N * N)
    cells = arr([1, 1, 1], np.int32)
    fam["ph"] = Family(
        {"m3g_ph_state_bytes": lambda r: lib.m3g_ph_state_bytes(C.byref(ph), r)},
        {"m3g_ph_init": lambda st, n, d: lib.m3g_ph_init(C.byref(ph), offsets, cells, lattice, positions, masses, 0.01, st, n, None),
         "m3g_ph_displace": lambda st, n, d: lib.m3g_ph_displace(C.byref(ph), st, n, DUMMY, None),
         "m3g_ph_force_constants": lambda st, n, d: lib.m3g_ph_force_constants(C.byref(ph), st, n, DUMMY, 1, DUMMY, DUMMY, DUMMY, None),
         "m3g_ph_dynmat": lambda st, n, d: lib.m3g_ph_dynmat(C.byref(ph), st, n, DUMMY, 1, DUMMY, DUMMY, N, DUMMY, None),
         "m3g_ph_dynmat_gradient": lambda st, n, d: lib.m3g_ph_dynmat_gradient(C.byref(ph), st, n, DUMMY, 1, DUMMY, DUMMY, N, DUMMY, None)})

    eos = _l.M3GElSizes(n_structs=S, n_atoms=N, n_deform=4, mode=_l.EL_MODE_EOS)
    elastic = _l.M3GElSizes(n_structs=S, n_atoms=N, n_deform=4, mode=_l.EL_MODE_ELASTIC)
    comps, mags = arr([_l.EL_VOLUMETRIC] * 4, np.int32), arr([-0.02, -0.01, 0.01, 0.02], np.float64)
    fam["el"] = Family(
        {"m3g_el_state_bytes": lambda r: lib.m3g_el_state_bytes(C.byref(eos), r)},
        {"m3g_el_init": lambda st, n, d: lib.m3g_el_init(C.byref(eos), offsets, lattice, positions, comps, mags, st, n, None),
         "m3g_el_deform": lambda st, n, d: lib.m3g_el_deform(C.byref(eos), st, n, DUMMY, DUMMY, None),
         "m3g_el_fit_elastic": lambda st, n, d: lib.m3g_el_fit_elastic(C.byref(elastic), st, n, DUMMY, DUMMY, DUMMY, None),
         "m3g_el_fit_eos": lambda st, n, d: lib.m3g_el_fit_eos(C.byref(eos), st, n, DUMMY, DUMMY, DUMMY, None)})

    traj, tp = _l.M3GTrajSizes(n_atoms=N, n_structs=S, max_species=1, rdf_bins=0, n_lags=1), _l.M3GTrajParams(r_max=1.0, remove_com=0)
    species = arr([0] * N, np.int32)
    fam["traj"] = Family(
        {"m3g_traj_state_bytes": lambda r: lib.m3g_traj_state_bytes(C.byref(traj), r)},
        {"m3g_traj_init": lambda st, n, d: lib.m3g_traj_init(C.byref(traj), C.byref(tp), offsets, species, masses, st, n, None),
         "m3g_traj_sample": lambda st, n, d: lib.m3g_traj_sample(C.byref(traj), C.byref(tp), st, n, DUMMY, None, DUMMY, None, 0.0, None),
         "m3g_traj_read": lambda st, n, d: lib.m3g_traj_read(C.byref(traj), st, n, *[None] * 7, None),
         "m3g_traj_frame": lambda st, n, d: lib.m3g_traj_frame(C.byref(traj), st, n, 0, DUMMY, DUMMY, None)})

    nma = _l.M3GNmaSizes(n_atoms=1, n_structs=1, n_unit_atoms=1, n_qpoints=1, n_modes=3, n_eig=9, n_phase=1, max_n=3, n_lags=0)
    npar = _l.M3GNmaParams(remove_com=0, reserved=0)
    one, frac, q, eig = arr([0, 1], np.int64), arr([0.0, 0.0, 0.0], np.float64), arr([0.0, 0.0, 0.0], np.float64), arr(np.zeros(18), np.float64)
    fam["nma"] = Family(
        {"m3g_nma_state_bytes": lambda r: lib.m3g_nma_state_bytes(C.byref(nma), r)},
        {"m3g_nma_init": lambda st, n, d: lib.m3g_nma_init(C.byref(nma), C.byref(npar), one, cells, lattice, frac, masses, one, q, eig, st, n, None),
         "m3g_nma_sample": lambda st, n, d: lib.m3g_nma_sample(C.byref(nma), C.byref(npar), st, n, DUMMY, DUMMY, None, 0.0, None),
         "m3g_nma_read": lambda st, n, d: lib.m3g_nma_read(C.byref(nma), st, n, *[None] * 7, None),
         "m3g_nma_frame": lambda st, n, d: lib.m3g_nma_frame(C.byref(nma), st, n, DUMMY, DUMMY, None)})

    ladder = arr([0, 2], np.int64)
    fam["remd"] = Family(
        {"m3g_remd_state_bytes": lambda r: lib.m3g_remd_state_bytes(2, 1, r), "m3g_remd_target_view": lambda r: lib.m3g_remd_target_view(N, 2, r)},
        {"m3g_remd_init": lambda st, n, d: lib.m3g_remd_init(2, 1, ladder, temps, seeds, st, n, None),
         "m3g_remd_exchange": lambda st, n, d: lib.m3g_remd_exchange(N, 2, 1, st, n, DUMMY, d, DUMMY, None, 0, None),
         "m3g_remd_read": lambda st, n, d: lib.m3g_remd_read(2, 1, st, n, *[None] * 9, None)},
        borrows=("m3g_remd_exchange",))
    fam["remd"].dyn_sizes = (N, 2)

    fam["mc"] = Family(
        {"m3g_mc_state_bytes": lambda r: lib.m3g_mc_state_bytes(N, S, r)},
        {"m3g_mc_init": lambda st, n, d: lib.m3g_mc_init(N, S, offsets, temps, seeds, ones8, st, n, None),
         "m3g_mc_propose": lambda st, n, d: lib.m3g_mc_propose(N, S, st, n, DUMMY, DUMMY, d, DUMMY, None),
         "m3g_mc_decide": lambda st, n, d: lib.m3g_mc_decide(N, S, st, n, DUMMY, DUMMY, d, DUMMY, None, None, DUMMY, None, None, None, 0, None),
         "m3g_mc_read": lambda st, n, d: lib.m3g_mc_read(N, S, st, n, *[None] * 9, None)},
        borrows=("m3g_mc_propose", "m3g_mc_decide"))

    rn = _l.M3GRnemdParams(kind=_l.RNEMD_HEAT, axis=2, flow_axis=0, n_slabs=2, n_swaps=1, reserved=0)
    fam["rnemd"] = Family(
        {"m3g_rnemd_state_bytes": lambda r: lib.m3g_rnemd_state_bytes(N, S, 2, r)},
        {"m3g_rnemd_init": lambda st, n, d: lib.m3g_rnemd_init(C.byref(rn), N, S, offsets, lattice, None, st, n, None),
         "m3g_rnemd_exchange": lambda st, n, d: lib.m3g_rnemd_exchange(C.byref(rn), N, S, st, n, DUMMY, d, DUMMY, 1, 1, None),
         "m3g_rnemd_read": lambda st, n, d: lib.m3g_rnemd_read(C.byref(rn), N, S, st, n, *[None] * 7, None)},
        borrows=("m3g_rnemd_exchange",))

    meta = _l.M3GMetaParams(n_cv=1, reserved=0, max_hills=0)
    meta.kind[0] = _l.CV_DISTANCE
    groups, member, weights = arr([0, 1], np.int64), arr([1, 2, 2], np.uint8), arr([1.0] * N, np.float64)
    sigma, height, inv_kdt, counts = arr([0.1], np.float64), arr([0.01], np.float64), arr([0.0], np.float64), arr([0], np.int64)
    fam["meta"] = Family(
        {"m3g_meta_state_bytes": lambda r: lib.m3g_meta_state_bytes(N, S, 1, 1, 0, r),
         "m3g_meta_state_view": lambda r: lib.m3g_meta_state_view(N, S, 1, 1, 0, r)},
        {"m3g_meta_init": lambda st, n, d: lib.m3g_meta_init(C.byref(meta), N, S, 1, offsets, groups, lattice, member, weights, None, None, None,
                                                             None, sigma, height, inv_kdt, st, n, None),
         "m3g_meta_bias": lambda st, n, d: lib.m3g_meta_bias(C.byref(meta), N, S, 1, st, n, DUMMY, DUMMY, DUMMY, 0, None, None),
         "m3g_meta_set_hills": lambda st, n, d: lib.m3g_meta_set_hills(C.byref(meta), N, S, 1, st, n, groups, counts, DUMMY, DUMMY, None),
         "m3g_meta_read": lambda st, n, d: lib.m3g_meta_read(C.byref(meta), N, S, 1, st, n, *[None] * 5, None)})
    for f in fam.values():
        f.keep = keep
    return _l, lib, fam


def observe():
    """Every case of this file against the loaded library: {case id: (status, message)}."""
    _l, lib, fam = _families()
    seen = {}

    def note(case, status):
        seen[case] = (status, lib.m3g_last_error().decode() if status else "")

    for f in fam.values():
        need = C.c_size_t()
        first = next(iter(f.bytes_calls))
        assert f.bytes_calls[first](C.byref(need)) == _l.M3G_OK and need.value > 0, first
        dyn = C.c_size_t()
        assert lib.m3g_dyn_state_bytes(*getattr(f, "dyn_sizes", (N, S)), C.byref(dyn)) == _l.M3G_OK
        for entry, call in f.bytes_calls.items():
            note(f"{entry}: null result", call(None))
        for entry, call in f.calls.items():
            note(f"{entry}: null state", call(None, BIG, BIG))
            note(f"{entry}: short state", call(DUMMY, need.value - 1, BIG))
        for entry in f.borrows:
            note(f"{entry}: short dynamics state", f.calls[entry](DUMMY, need.value, dyn.value - 1))
    return seen


EL_SIZES = "bad sizes (need 1 <= n_structs <= n_atoms, 1 <= n_deform <= M3G_EL_MAX_DEFORM, mode 0 / 1)"
PH_SIZES = "bad sizes (need 1 <= n_structs <= n_unit_atoms <= n_super_atoms <= n_pairs)"
EXPECTED = {   # 1 = M3G_ERR_VALUE, 3 = M3G_ERR_SIZE
    'm3g_fire_state_bytes: null result': (1, 'm3g_fire_state_bytes: bad sizes'),
    'm3g_fire_init: null state': (1, 'm3g_fire_init: null argument or bad sizes'),
    'm3g_fire_init: short state': (3, 'm3g_fire_init: state buffer too small (3839 < 3840)'),
    'm3g_fire_step: null state': (1, 'm3g_fire_step: null argument or bad sizes'),
    'm3g_fire_step: short state': (3, 'm3g_fire_step: state buffer too small'),
    'm3g_fire_read: null state': (1, 'm3g_fire_read: null argument or bad sizes'),
    'm3g_fire_read: short state': (3, 'm3g_fire_read: state buffer too small'),
    'm3g_lbfgs_state_bytes: null result': (1, 'm3g_lbfgs_state_bytes: bad sizes (1 <= memory <= 2047)'),
    'm3g_lbfgs_init: null state': (1, 'm3g_lbfgs_init: null argument or bad sizes'),
    'm3g_lbfgs_init: short state': (3, 'm3g_lbfgs_init: state buffer too small (7679 < 7680)'),
    'm3g_lbfgs_step: null state': (1, 'm3g_lbfgs_step: null argument or bad sizes'),
    'm3g_lbfgs_step: short state': (3, 'm3g_lbfgs_step: state buffer too small'),
    'm3g_lbfgs_read: null state': (1, 'm3g_lbfgs_read: null argument or bad sizes'),
    'm3g_lbfgs_read: short state': (3, 'm3g_lbfgs_read: state buffer too small'),
    'm3g_neb_state_bytes: null result': (1, 'm3g_neb_state_bytes: bad sizes (need 1 <= n_bands <= n_images <= n_atoms)'),
    'm3g_neb_init: null state': (1, 'm3g_neb_init: null argument or bad sizes (need 1 <= n_bands <= n_images <= n_atoms)'),
    'm3g_neb_init: short state': (3, 'm3g_neb_init: state buffer too small (3327 < 3328)'),
    'm3g_neb_forces: null state': (1, 'm3g_neb_forces: null argument or bad sizes'),
    'm3g_neb_forces: short state': (3, 'm3g_neb_forces: state buffer too small'),
    'm3g_ph_state_bytes: null result': (1, 'm3g_ph_state_bytes: ' + PH_SIZES),
    'm3g_ph_init: null state': (1, 'm3g_ph_init: null argument or ' + PH_SIZES),
    'm3g_ph_init: short state': (3, 'm3g_ph_init: state buffer too small (8447 < 8448)'),
    'm3g_ph_displace: null state': (1, 'm3g_ph_displace: null argument or bad sizes'),
    'm3g_ph_displace: short state': (3, 'm3g_ph_displace: state buffer too small'),
    'm3g_ph_force_constants: null state': (1, 'm3g_ph_force_constants: null argument, bad sizes or asr not 0 / 1'),
    'm3g_ph_force_constants: short state': (3, 'm3g_ph_force_constants: state buffer too small'),
    'm3g_ph_dynmat: null state': (1, 'm3g_ph_dynmat: null argument, bad sizes, n_q < 0 or max_unit_atoms outside [1, n_unit_atoms]'),
    'm3g_ph_dynmat: short state': (3, 'm3g_ph_dynmat: state buffer too small'),
    'm3g_ph_dynmat_gradient: null state': (1, 'm3g_ph_dynmat_gradient: null argument, bad sizes, n_q < 0 or max_unit_atoms outside [1, n_unit_atoms]'),
    'm3g_ph_dynmat_gradient: short state': (3, 'm3g_ph_dynmat_gradient: state buffer too small'),
    'm3g_el_state_bytes: null result': (1, 'm3g_el_state_bytes: ' + EL_SIZES),
    'm3g_el_init: null state': (1, 'm3g_el_init: null argument or ' + EL_SIZES),
    'm3g_el_init: short state': (3, 'm3g_el_init: state buffer too small (2047 < 2048)'),
    'm3g_el_deform: null state': (1, 'm3g_el_deform: null argument or ' + EL_SIZES),
    'm3g_el_deform: short state': (3, 'm3g_el_deform: state buffer too small'),
    'm3g_el_fit_elastic: null state': (1, 'm3g_el_fit_elastic: null argument or ' + EL_SIZES),
    'm3g_el_fit_elastic: short state': (3, 'm3g_el_fit_elastic: state buffer too small'),
    'm3g_el_fit_eos: null state': (1, 'm3g_el_fit_eos: null argument or ' + EL_SIZES),
    'm3g_el_fit_eos: short state': (3, 'm3g_el_fit_eos: state buffer too small'),
    'm3g_traj_state_bytes: null result': (1, 'm3g_traj_state_bytes: null argument'),
    'm3g_traj_init: null state': (1, 'm3g_traj_init: null argument'),
    'm3g_traj_init: short state': (3, 'm3g_traj_init: state buffer too small (4351 < 4352)'),
    'm3g_traj_sample: null state': (1, 'm3g_traj_sample: null argument'),
    'm3g_traj_sample: short state': (3, 'm3g_traj_sample: state buffer too small'),
    'm3g_traj_read: null state': (1, 'm3g_traj_read: null argument'),
    'm3g_traj_read: short state': (3, 'm3g_traj_read: state buffer too small'),
    'm3g_traj_frame: null state': (1, 'm3g_traj_frame: null argument or no ring (n_lags == 0)'),
    'm3g_traj_frame: short state': (3, 'm3g_traj_frame: state buffer too small'),
    'm3g_nma_state_bytes: null result': (1, 'm3g_nma_state_bytes: null argument'),
    'm3g_nma_init: null state': (1, 'm3g_nma_init: null argument'),
    'm3g_nma_init: short state': (3, 'm3g_nma_init: state buffer too small (6911 < 6912)'),
    'm3g_nma_sample: null state': (1, 'm3g_nma_sample: null argument'),
    'm3g_nma_sample: short state': (3, 'm3g_nma_sample: state buffer too small'),
    'm3g_nma_read: null state': (1, 'm3g_nma_read: null argument'),
    'm3g_nma_read: short state': (3, 'm3g_nma_read: state buffer too small'),
    'm3g_nma_frame: null state': (1, 'm3g_nma_frame: null argument'),
    'm3g_nma_frame: short state': (3, 'm3g_nma_frame: state buffer too small'),
    'm3g_remd_state_bytes: null result': (1, 'm3g_remd_state_bytes: null argument or bad sizes'),
    'm3g_remd_target_view: null result': (1, 'm3g_remd_target_view: null argument or bad sizes'),
    'm3g_remd_init: null state': (1, 'm3g_remd_init: null argument or bad sizes'),
    'm3g_remd_init: short state': (3, 'm3g_remd_init: state buffer too small (3583 < 3584)'),
    'm3g_remd_exchange: null state': (1, 'm3g_remd_exchange: null argument or bad sizes'),
    'm3g_remd_exchange: short state': (3, 'm3g_remd_exchange: replica-exchange state buffer too small'),
    'm3g_remd_read: null state': (1, 'm3g_remd_read: null argument or bad sizes'),
    'm3g_remd_read: short state': (3, 'm3g_remd_read: state buffer too small'),
    'm3g_remd_exchange: short dynamics state': (3, 'm3g_remd_exchange: dynamics state buffer too small'),
    'm3g_mc_state_bytes: null result': (1, 'm3g_mc_state_bytes: null argument or bad sizes'),
    'm3g_mc_init: null state': (1, 'm3g_mc_init: null argument or bad sizes'),
    'm3g_mc_init: short state': (3, 'm3g_mc_init: state buffer too small (4863 < 4864)'),
    'm3g_mc_propose: null state': (1, 'm3g_mc_propose: null argument or bad sizes'),
    'm3g_mc_propose: short state': (3, 'm3g_mc_propose: Monte Carlo state buffer too small'),
    'm3g_mc_decide: null state': (1, 'm3g_mc_decide: null argument or bad sizes'),
    'm3g_mc_decide: short state': (3, 'm3g_mc_decide: Monte Carlo state buffer too small'),
    'm3g_mc_read: null state': (1, 'm3g_mc_read: null argument or bad sizes'),
    'm3g_mc_read: short state': (3, 'm3g_mc_read: state buffer too small'),
    'm3g_mc_propose: short dynamics state': (3, 'm3g_mc_propose: dynamics state buffer too small'),
    'm3g_mc_decide: short dynamics state': (3, 'm3g_mc_decide: dynamics state buffer too small'),
    'm3g_rnemd_state_bytes: null result': (1, 'm3g_rnemd_state_bytes: null argument or bad sizes'),
    'm3g_rnemd_init: null state': (1, 'm3g_rnemd_init: null argument or bad sizes'),
    'm3g_rnemd_init: short state': (3, 'm3g_rnemd_init: state buffer too small (4351 < 4352)'),
    'm3g_rnemd_exchange: null state': (1, 'm3g_rnemd_exchange: null argument or bad sizes'),
    'm3g_rnemd_exchange: short state': (3, 'm3g_rnemd_exchange: rNEMD state buffer too small'),
    'm3g_rnemd_read: null state': (1, 'm3g_rnemd_read: null argument or bad sizes'),
    'm3g_rnemd_read: short state': (3, 'm3g_rnemd_read: state buffer too small'),
    'm3g_rnemd_exchange: short dynamics state': (3, 'm3g_rnemd_exchange: dynamics state buffer too small'),
    'm3g_meta_state_bytes: null result': (1, 'm3g_meta_state_bytes: null argument or bad sizes (1 <= n_groups <= n_structs <= n_atoms, n_cv 1 .. 2, '
                                             'max_hills >= 0)'),
    'm3g_meta_state_view: null result': (1, 'm3g_meta_state_view: null argument or bad sizes'),
    'm3g_meta_init: null state': (1, 'm3g_meta_init: null argument'),
    'm3g_meta_init: short state': (3, 'm3g_meta_init: state buffer too small (5887 < 5888)'),
    'm3g_meta_bias: null state': (1, 'm3g_meta_bias: null argument or bad sizes'),
    'm3g_meta_bias: short state': (3, 'm3g_meta_bias: state buffer too small'),
    'm3g_meta_set_hills: null state': (1, 'm3g_meta_set_hills: null argument or bad sizes'),
    'm3g_meta_set_hills: short state': (3, 'm3g_meta_set_hills: state buffer too small'),
    'm3g_meta_read: null state': (1, 'm3g_meta_read: null argument or bad sizes'),
    'm3g_meta_read: short state': (3, 'm3g_meta_read: state buffer too small'),
}


def test_every_shared_refusal_keeps_its_status_and_text():
    seen = observe()
    assert sorted(seen) == sorted(EXPECTED)
    wrong = {case: (seen[case], EXPECTED[case]) for case in EXPECTED if seen[case] != EXPECTED[case]}
    assert not wrong, wrong


def test_the_table_covers_every_entry_point_of_the_eleven_families():
    _l, lib, fam = _families()
    prefixes = ("m3g_fire_", "m3g_lbfgs_", "m3g_neb_", "m3g_ph_", "m3g_el_", "m3g_traj_", "m3g_nma_", "m3g_remd_", "m3g_mc_", "m3g_rnemd_",
                "m3g_meta_")
    bound = {name for name in _l.SYMBOLS if name.startswith(prefixes)}
    covered = {entry for f in fam.values() for entry in list(f.bytes_calls) + list(f.calls)}
    assert len(bound) == 53 and bound - covered == {"m3g_ph_group_velocities"} and covered <= bound
    status = {case.split(": ")[1]: set() for case in EXPECTED if ": " in case}
    for case, (code, _) in EXPECTED.items():
        status[case.split(": ")[1]].add(code)
    assert status["null result"] == status["null state"] == {_l.M3G_ERR_VALUE}
    assert status["short state"] == status["short dynamics state"] == {_l.M3G_ERR_SIZE}
