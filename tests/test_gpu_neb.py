"""Batched climbing-image NEB on the MI355X (torch_m3gnet.neb, C ABI m3g_neb_*): the projection against the numpy restatement
(tests/neb_reference.py) over every tangent branch, the device band loop on the Mueller-Brown surface in lockstep with the restatement
and onto the saddle, bitwise independence of the batch, non-finite forces, graph capture, and vacancy hops under the LJ-fitted model."""
import numpy as np
import pytest
import torch

import fire_reference as fr
import neb_reference as nr
from helpers import GOLDEN
from test_neb_cpu import mb_band, mb_image, mb_saddle, mueller_brown

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- synthetic bands --------------------------------------------------------------------------------------------------------
def _images(n_int, n, seed):
    """M = n_int + 2 images [n,3] of one band: a random start moved along a random direction, with noise."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 10, (n, 3))
    step = rng.normal(0, 0.3, (n, 3))
    return [base + j * step + rng.normal(0, 0.05, (n, 3)) for j in range(n_int + 2)]


def _inputs(n_int, n, seed, it, ties=False):
    """Energies [M] (endpoints first and last; with `ties` drawn from four levels, so that ties and flat triples are common) and
    interior forces [n_int, n, 3], float32 values."""
    rng = np.random.default_rng([seed, it])
    if ties:
        e = rng.integers(0, 4, n_int + 2).astype(np.float32) * np.float32(0.25) - np.float32(3.0)
    else:
        e = rng.normal(-3.0, 0.5, n_int + 2).astype(np.float32)
    f = rng.normal(0, 1, (n_int, n, 3)).astype(np.float32)
    return e, f


def _state(specs, imgs, ep_energies, k, climb):
    from torch_m3gnet.neb import NEBState

    image_offsets = np.concatenate([[0], np.cumsum([n for n_int, n in specs for _ in range(n_int)])])
    band_images = np.concatenate([[0], np.cumsum([n_int for n_int, _ in specs])])
    ep = torch.tensor(np.concatenate([p for band in imgs for p in (band[0], band[-1])]), dtype=torch.float64, device=DEV)
    return NEBState(image_offsets, band_images, k, climb, ep, np.asarray(ep_energies).reshape(-1, 2))


def _branch(vp, v, vn):
    if vn > v > vp:
        return "rise"
    if vn < v < vp:
        return "fall"
    if vp == v == vn:
        return "flat"
    return ("tie-" if vp == v or v == vn or vp == vn else "") + ("up" if vn > vp else "down")


def _ulp_equal(dev, ref64):
    ref = ref64.astype(np.float32)
    both_nan = np.isnan(dev) & np.isnan(ref)
    close = np.abs(dev.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)
    return bool((both_nan | close).all())


SPECS = [(1, 1), (3, 32), (7, 1000), (3, 10000), (7, 1), (1, 32)]


def test_projection_matches_restatement_over_every_branch():
    from torch_m3gnet.neb import neb_forces

    imgs = [_images(n_int, n, 100 + b) for b, (n_int, n) in enumerate(SPECS)]
    branches = set()
    for trial in range(8):
        climb = [(b + trial) % 2 for b in range(len(SPECS))]
        k = [0.1 * (1 + b) for b in range(len(SPECS))]
        ins = [_inputs(n_int, n, b, trial, ties=True) for b, (n_int, n) in enumerate(SPECS)]
        st = _state(SPECS, imgs, [(e[0], e[-1]) for e, _ in ins], k, climb)
        pos = torch.tensor(np.concatenate([p for band in imgs for p in band[1:-1]]), dtype=torch.float64, device=DEV)
        energies = torch.tensor(np.concatenate([e[1:-1] for e, _ in ins]), device=DEV)
        forces = torch.tensor(np.concatenate([f.reshape(-1, 3) for _, f in ins]), device=DEV)
        neb_forces(st, pos, energies, forces)
        torch.cuda.synchronize()
        dev_f, dev_rows = st.forces.cpu().numpy(), st.rows.cpu().numpy()
        a = i = 0
        for b, (n_int, n) in enumerate(SPECS):
            e, f = ins[b]
            ref_f, ref_rows = nr.neb_forces(imgs[b], e.astype(np.float64), f, k[b], bool(climb[b]))
            assert _ulp_equal(dev_f[a:a + n_int * n], ref_f.reshape(-1, 3)), (trial, b)
            rows = dev_rows[i:i + n_int]
            assert np.array_equal(rows[:, 4], ref_rows[:, 4]), (trial, b, rows[:, 4], ref_rows[:, 4])
            scale = np.maximum(np.nan_to_num(np.abs(ref_rows)).max(axis=0), 1.0)
            ok = np.isnan(ref_rows) & np.isnan(rows) | (np.abs(rows - ref_rows) <= 1e-12 * scale)
            assert ok.all(), (trial, b, rows, ref_rows)
            branches |= {_branch(e[j - 1], e[j], e[j + 1]) for j in range(1, n_int + 1)}
            a, i = a + n_int * n, i + n_int
    assert {"rise", "fall", "up", "down", "flat"} <= branches and any(x.startswith("tie-") for x in branches), branches


# ---- the device band loop --------------------------------------------------------------------------------------------------
def test_mueller_brown_band_loop_matches_restatement_and_finds_the_saddle():
    from torch_m3gnet.neb import neb_forces
    from torch_m3gnet.relax import FireState, fire_step

    imgs = mb_band()
    M, fmax = len(imgs), 1e-4
    e0, e1 = (float(np.float32(mb_image(p)[0])) for p in (imgs[0], imgs[-1]))
    st = _state([(M - 2, 1)], [imgs], [(e0, e1)], 0.1, 1)
    pos = torch.tensor(np.concatenate(imgs[1:-1]), dtype=torch.float64, device=DEV)
    fire = FireState(pos, None, st.band_offsets, relax_cell=False, fmax=fmax)
    ref = nr.BandReference(imgs, (e0, e1), k=0.1, climb=True, fmax=fmax)
    for it in range(2000):
        p = pos.cpu().numpy()
        ev = [mb_image(x[None]) for x in p]
        e = np.array([x for x, _ in ev], dtype=np.float32)
        f = np.concatenate([x for _, x in ev]).astype(np.float32)
        neb_forces(st, pos, torch.tensor(e, device=DEV), torch.tensor(f, device=DEV))
        fire_step(fire, st.forces)
        if it < 40:   # lockstep with the restatement, fed the same float32 energies and forces
            ref.step(e.astype(np.float64), f.astype(np.float64).reshape(M - 2, 1, 3))
            got = pos.cpu().numpy()
            assert np.abs(got - np.concatenate(ref.images[1:-1])).max() < 1e-12, it
            assert _ulp_equal(st.forces.cpu().numpy(), ref.neb_forces.reshape(-1, 3)), it
        torch.cuda.synchronize()
        if fire.n_unconverged == 0:
            break
    r = fire.read()
    assert r["flags"][0] & fr.CONVERGED and not r["flags"][0] & fr.ERROR and r["n_steps"][0] > 40
    rows = st.rows.cpu().numpy()
    ci = int(np.flatnonzero(rows[:, 4] == 1.0)[0])
    p = pos.cpu().numpy()
    s = mb_saddle(p[ci])
    assert np.linalg.norm(p[ci] - s) < 1e-3 and abs(mueller_brown(p[ci])[0] - mueller_brown(s)[0]) < 1e-5
    assert abs(s[0] / 2.0 - 0.212) < 2e-3 and abs(s[1] / 2.0 - 0.293) < 2e-3


def _run(specs, seeds, iters, fmax=1e-6, nan_at=None, capture=False):
    """The device loop of neb_forces + fire_step over synthetic bands (inputs independent of the positions): per-band inputs from
    (seed, iteration), so a band sees the same inputs alone and in a batch."""
    from torch_m3gnet.neb import neb_forces
    from torch_m3gnet.relax import FireState, fire_step

    imgs = [_images(n_int, n, s) for (n_int, n), s in zip(specs, seeds)]
    e_ep = [_inputs(n_int, n, s, 0)[0][[0, -1]] for (n_int, n), s in zip(specs, seeds)]
    st = _state(specs, imgs, e_ep, 0.5, 1)
    pos = torch.tensor(np.concatenate([p for band in imgs for p in band[1:-1]]), dtype=torch.float64, device=DEV)
    fire = FireState(pos, None, st.band_offsets, relax_cell=False, fmax=fmax)
    snaps = []
    for it in range(iters):
        ins = [_inputs(n_int, n, s, it if not capture else 1) for (n_int, n), s in zip(specs, seeds)]
        e = np.concatenate([x[1:-1] for x, _ in ins])
        f = np.concatenate([x.reshape(-1, 3) for _, x in ins])
        if nan_at is not None and it == nan_at[0]:
            f[nan_at[1], 2] = np.nan
        neb_forces(st, pos, torch.tensor(e, device=DEV), torch.tensor(f, device=DEV))
        fire_step(fire, st.forces)
        snaps.append(pos.cpu().numpy())
    torch.cuda.synchronize()
    return st, fire, pos, snaps


def _band_rows(specs, b):
    sizes = [n_int * n for n_int, n in specs]
    return slice(sum(sizes[:b]), sum(sizes[:b + 1]))


def test_band_alone_and_in_a_batch_give_identical_bits():
    specs, seeds = [(1, 1000), (3, 32), (5, 7)], [11, 12, 13]
    st_b, fb, pb, _ = _run(specs, seeds, 30)
    for b in range(3):
        st_a, fa, pa, _ = _run([specs[b]], [seeds[b]], 30)
        rows = _band_rows(specs, b)
        assert torch.equal(pa, pb[rows]), b
        assert torch.equal(st_a.forces, st_b.forces[rows]), b
        ra, rb = fa.read(), fb.read()
        assert ra["n_steps"][0] == rb["n_steps"][b] == 30 and ra["dt"][0] == rb["dt"][b]


def test_non_finite_force_fails_that_band_only():
    from torch_m3gnet import _lib

    specs, seeds = [(3, 32), (3, 32)], [21, 22]
    st, fire, pos, snaps = _run(specs, seeds, 12, nan_at=(5, 32 + 7))   # band 0, its second interior image
    r = fire.read()
    assert r["flags"][0] & _lib.FIRE_ERROR and not r["flags"][1] & _lib.FIRE_ERROR
    assert list(r["n_steps"]) == [5, 12]
    for s in snaps[5:]:
        assert np.array_equal(s[:96], snaps[4][:96])   # frozen where it stood
    _, _, pos1, _ = _run([specs[1]], [seeds[1]], 12)
    assert torch.equal(pos1, pos[96:]) and torch.isfinite(pos).all()


def test_neb_and_fire_capture_replays_bitwise():
    from torch_m3gnet.neb import neb_forces
    from torch_m3gnet.relax import FireState, fire_step

    specs, seeds = [(3, 32), (1, 1000)], [31, 32]
    eager_st, eager_fire, eager_pos, _ = _run(specs, seeds, 10, capture=True)
    imgs = [_images(n_int, n, s) for (n_int, n), s in zip(specs, seeds)]
    e_ep = [_inputs(n_int, n, s, 0)[0][[0, -1]] for (n_int, n), s in zip(specs, seeds)]
    st = _state(specs, imgs, e_ep, 0.5, 1)
    pos = torch.tensor(np.concatenate([p for band in imgs for p in band[1:-1]]), dtype=torch.float64, device=DEV)
    fire = FireState(pos, None, st.band_offsets, relax_cell=False, fmax=1e-6)
    ins = [_inputs(n_int, n, s, 1) for (n_int, n), s in zip(specs, seeds)]
    e = torch.tensor(np.concatenate([x[1:-1] for x, _ in ins]), device=DEV)
    f = torch.tensor(np.concatenate([x.reshape(-1, 3) for _, x in ins]), device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        neb_forces(st, pos, e, f)
        fire_step(fire, st.forces)
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pos, eager_pos) and torch.equal(st.forces, eager_st.forces) and torch.equal(st.rows, eager_st.rows)
    assert fire.read()["n_steps"].tolist() == eager_fire.read()["n_steps"].tolist() == [10, 10]


# ---- vacancy hops under the LJ-fitted model -------------------------------------------------------------------------------------
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def _model():
    from torch_m3gnet.model.build import build_model_from_npz

    return build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)


def _hop(a, mover=1):
    """2x2x2 fcc Cu without site 0; the atom on site `mover` (a nearest neighbour of site 0) hops into the vacancy."""
    from torch_m3gnet.neb import interpolate

    grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    sites = (grid + FCC_BASE[None]).reshape(-1, 3) * a
    lat = np.eye(3) * 2 * a
    init = sites[1:].copy()
    final = init.copy()
    final[mover - 1] = sites[0]
    return lat, np.full(31, 29), interpolate(lat, init, final, 7)


def test_vacancy_hop_under_the_fitted_model():
    from torch_m3gnet.neb import NEB

    neb = NEB(_model())
    kw = dict(fmax=0.02, steps=500, relax_endpoints=True, endpoint_fmax=0.005)
    bands = [_hop(3.60), _hop(3.65, mover=2)]
    (alone,) = neb.run([bands[0]], **kw)
    assert alone["converged"] and not alone["error"] and alone["climbing_image"] == 3, (alone["n_steps"], alone["energies"])
    assert np.sqrt((alone["forces"][2] ** 2).sum(1).max()) < 0.02
    e = alone["energies"]
    assert np.abs(e - e[::-1]).max() < 1e-4, e - e[::-1]
    assert alone["barrier_forward"] > 0 and e.argmax() == 3
    assert abs(alone["barrier_forward"] - (e[3] - e[0])) < 1e-12 and abs(alone["barrier_backward"] - (e[3] - e[6])) < 1e-12
    together = neb.run(bands, **kw)
    (second,) = neb.run([bands[1]], **kw)
    for one, t in zip((alone, second), together):
        assert t["converged"] and one["converged"] and t["climbing_image"] == one["climbing_image"]
        assert np.abs(one["energies"] - t["energies"]).max() / 31 < 1e-5
        assert np.abs(one["positions"] - t["positions"]).max() < 1e-4


def test_out_of_range_species_raises():
    from torch_m3gnet.neb import NEB

    lat, z, imgs = _hop(3.6)
    z = z.copy()
    z[3] = 200
    with pytest.raises((IndexError, ValueError)):
        NEB(_model()).run([(lat, z, imgs)], steps=3)
