"""Where the kernels write, and what they read before anything wrote it: the energy/force step, the ten driver states and the
capacity buffers of m3g_md_step on buffers of EXACTLY the size the library reports, each between two 1 MiB guard bands
(tests/guarded.py), once with 0x00 and once with 0xFF (NaN / -1) inside.

Held to exact size here: the topology buffer (m3g_topology_bytes), the workspace (m3g_workspace_bytes), every output and input of
m3g_io; the states of FIRE, L-BFGS, dyn, nhc, REMD, swap MC, NEB, phonons, elasticity and trajectory (m3g_*_state_bytes, through
_driver.state_tensor); and the eight capacity buffers of VerletGraph._md_prepare (through data.md._alloc).

Every case asserts: all bands intact under both fills; results bitwise equal between the fills and to the plain call on torch's own
buffers; and, in the 0xFF run, no NaN in any output -- every element of every output is 0xFFFFFFFF before the call, which is a NaN,
so a NaN-free output was written everywhere, and the 0x00 run, bitwise equal to it, was too.  (An element left holding 0x00 cannot
be told from a computed zero on its own; the equality with the 0xFF run is what covers it.)

The method sees stray writes within 1 MiB of a buffer and nothing farther away; it does not see stray reads that reach no output.

What it found when it was written: no band was ever damaged and no result depended on the fill -- except that the vector-ALU
baseline (edge_kernel = 0) was not bitwise reproducible at all, whatever its buffers held: its edge kernel added each wave's partial
message sums onto the centre atoms with float atomics, so x, edge_attr, forces and stresses moved in the last bits from run to run
(n17: 2,303 of 39,296 edge_attr values between two plain calls).  The kernel now stores the message rows and a second launch sums
each centre's rows in list order; edge_kernel = 0 passes the same bitwise assertions as every other selection."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from guarded import Arena
from helpers import PERSISTENT, PERSISTENT_TAIL, random_cell_graph, record_line
from test_gpu_dynamics import _fcc

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = "guard_bands.txt"
FILLS = (0x00, 0xFF)


def _K():
    from torch_m3gnet.data import MaterialGraphKey as K

    return K


def _bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes (torch.equal on floats calls -0.0 and 0.0 equal)."""
    return t.contiguous().view(-1).view(torch.uint8)


def _same_bits(a, b) -> bool:
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ================================================================== 1. the energy/force step
# (cutoff, three-body cutoff, l_max, n_max, num_types, width, blocks): the default architecture; that of `dense`, whose lists are built
# for cutoff = three-body cutoff = 6.0; and the two any-size models (the second: C = l_max * n_max = 90, the table's maximum)
DEFAULT = (5.0, 4.0, 3, 3, 95, 64, 3)
DENSE = (6.0, 6.0, 3, 3, 95, 64, 3)
ANY_A = (4.5, 4.0, 5, 4, 40, 96, 2)
ANY_B = (4.0, 3.5, 9, 10, 60, 24, 1)
BATCH9_SIZES = (20, 3, 11, 7, 1, 16, 2, 13, 5)   # S = 9 > kForceTailMaxStructs = 8; structure 4 is `lone`: empty segments inside every list


def _lone(cut, tb):
    from torch_m3gnet.data.material_graph import MaterialGraph

    return MaterialGraph.from_arrays(np.eye(3) * 20.0, [[10.0, 10.0, 10.0]], [29], cut, tb)


def _pair(cut, tb):
    from torch_m3gnet.data.material_graph import MaterialGraph

    return MaterialGraph.from_arrays(np.eye(3) * 20.0, [[10.0, 10.0, 10.0], [13.0, 10.0, 10.0]], [29, 8], cut, tb)


def _batch9(cut, tb):
    # seeds 0 .. 8, boxes of about 14 A^3 per atom and at least 5 A: E % 16 = 4, 8, 8 at the three cutoff pairs used here
    return [_lone(cut, tb) if n == 1 else random_cell_graph(n, max(5.0, (14.0 * n) ** (1 / 3)), s, cut, tb, zmax=39)
            for s, n in enumerate(BATCH9_SIZES)]


def _fcc864(cut, tb):
    from torch_m3gnet.data.material_graph import MaterialGraph

    pos, lat = _fcc(3.61, 6)
    pos = pos + np.random.default_rng(0).uniform(-0.01, 0.01, pos.shape)
    return MaterialGraph.from_arrays(lat, pos, np.full(len(pos), 29), cut, tb)


# name -> (builder of the structure list, what must hold of (N, E, T, S) at the default cutoffs); seeds chosen on the host so that no
# random shape has E % 16 == 0 and their E % 64 all differ (38, 30, 52, 18)
SHAPES = {
    "lone": (lambda c, t: [_lone(c, t)], dict(N=1, E=0, T=0, S=1)),
    "pair": (lambda c, t: [_pair(c, t)], dict(N=2, E=2, T=0, S=1)),
    "n17": (lambda c, t: [random_cell_graph(17, 6.2, 0, c, t, zmax=39)], dict(N=17, S=1, e64=38)),
    "n129": (lambda c, t: [random_cell_graph(129, 12.2, 1, c, t, zmax=39)], dict(N=129, S=1, e64=30)),
    "batch9": (_batch9, dict(N=78, S=9, e64=52)),
    "dense": (lambda c, t: [random_cell_graph(20, 6.5, 2, c, t, zmax=39)], dict(N=20, S=1, e64=18)),
    "fcc864": (lambda c, t: [_fcc864(c, t)], dict(N=864, E=36288, S=1)),
}
PART_FILLED = ("n17", "n129", "batch9", "dense")   # their last 16-edge tile is part-filled, at every cutoff pair they are built for


@functools.lru_cache(maxsize=None)
def _host_batch(shape: str, cut: float, tb: float):
    """The shape's batch on the host, built once per cutoff pair and never modified (every use clones it onto the device)."""
    from torch_m3gnet.data.material_graph import Batch

    return Batch.from_data_list(SHAPES[shape][0](cut, tb))


def _sizes(batch):
    K = _K()
    return (int(batch[K.POS].size(0)), int(batch[K.EDGE_INDEX].size(1)), int(batch[K.TRIPLET_EDGE_INDEX].size(1)), int(batch[K.LATTICE].size(0)))


@functools.lru_cache(maxsize=None)
def _model(arch: tuple):
    """One model per architecture for the whole module; every test puts the options it moved back in a `finally`."""
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(0)
    model = build_model(*arch, elemental_energies=torch.linspace(-3.0, -1.0, arch[4]), energy_scale=1.7)
    for m in model.model:
        if type(m).__name__ == "ThreeBodyInteration":
            m.nsb.factors = m.nsb.documented_factors()
    return model.to(DEV)


# the library's defaults of every option a selection moves (Options, csrc/m3g_step_path.h), in an order that restores them:
# small_tiles moves small_tiles_fwd with it, so the forward threshold comes after it
DEFAULTS = dict(precision=0, small_tiles=1536, small_tiles_fwd=3072, split_node_tiles=128, split_tail=1, rev_kernel=1, save_p1=1,
                save_p2=1, threebody_moments=1, dp1_by_dst=0, stress_mode=0, overlap=0, fuse_node_tb=1, small_launches=1, edge_kernel=1)
PRECISIONS = {"fp32": 0, "bf16x3": 1, "f16x3": 2}

# name -> (architecture or None for the shape's own default-architecture model, precision, options, want_forces, extras)
SELECTIONS = {}
for _prec in PRECISIONS:
    SELECTIONS[f"default-{_prec}"] = (None, _prec, {}, True, True)
    SELECTIONS[f"persistent-{_prec}"] = (None, _prec, PERSISTENT, True, True)
    SELECTIONS[f"persistent_tail-{_prec}"] = (None, _prec, PERSISTENT_TAIL, True, True)
for _name, _value in (("rev_kernel", 0), ("save_p2", 0), ("save_p1", 0), ("threebody_moments", 0), ("dp1_by_dst", 1), ("stress_mode", 1),
                      ("overlap", 1), ("fuse_node_tb", 0), ("small_launches", 0), ("edge_kernel", 0), ("edge_kernel", 2)):
    SELECTIONS[f"{_name}={_value}"] = (None, "fp32", {_name: _value}, True, True)
SELECTIONS["energy_only"] = (None, "fp32", {}, False, True)
SELECTIONS["energy_only-persistent"] = (None, "fp32", PERSISTENT, False, True)
SELECTIONS["no_extras"] = (None, "fp32", {}, True, False)
SELECTIONS["no_extras-persistent"] = (None, "fp32", PERSISTENT, True, False)
SELECTIONS["any_size-C20-w96"] = (ANY_A, "fp32", {}, True, True)
SELECTIONS["any_size-C90-w24"] = (ANY_B, "fp32", {}, True, True)
ANY_SIZE_SHAPES = ("lone", "n17", "batch9")   # the shapes the any-size models run on, rebuilt for their cutoffs

# every selection on every shape it accepts: resolve_step_path and the plan refuse none of the default-architecture selections on any
# of these shapes, so there is no skip in this table
STEP_CASES = [(shape, sel) for sel, spec in SELECTIONS.items() for shape in (SHAPES if spec[0] is None else ANY_SIZE_SHAPES)]


class Outputs(dict):
    """{key: output tensor} of one guarded step; `sizes`: N, E, T, S, workspace and topology bytes, for the record."""
    sizes: dict


def guarded_step(model, graph, fill, want_forces=True, extras=True):
    """One m3g_energy_forces call as Engine.run issues it, on buffers this test owns: topology of exactly m3g_topology_bytes (built into
    it with m3g_topology_build_hints), workspace of exactly m3g_workspace_bytes, every output of m3g_io, and guarded copies of the
    inputs; `fill` inside topology, workspace and outputs.  Bands checked after the build and after the call; the topology's
    status word must be 0.  `model(graph)` must have run once (it commits the plan).  Returns the outputs."""
    from torch_m3gnet import _cuda, _lib
    from torch_m3gnet.nn import modules as M

    K = _K()
    eng, lib, p = model.engine, model.engine.lib, M._ptr
    dev = graph[K.POS].device
    arena = Arena(dev)
    with _cuda.on_device(dev):
        inputs = {K.POS: graph[K.POS].detach().contiguous().float(), K.ATOM_TYPES: graph[K.ATOM_TYPES].contiguous().long(),
                  K.EDGE_CELL_SHIFT: graph[K.EDGE_CELL_SHIFT].contiguous().to(torch.int32), K.LATTICE: graph[K.LATTICE].contiguous().float(),
                  K.EDGE_INDEX: graph[K.EDGE_INDEX].contiguous().long(), K.TRIPLET_EDGE_INDEX: graph[K.TRIPLET_EDGE_INDEX].contiguous().long(),
                  K.BATCH: graph[K.BATCH].contiguous().long()}
        inp = {key: arena.take_copy(t, f"input {key}") for key, t in inputs.items()}
        originals = {key: t.clone() for key, t in inp.items()}
        N, E, T, S = int(inp[K.BATCH].numel()), int(inp[K.EDGE_INDEX].size(1)), int(inp[K.TRIPLET_EDGE_INDEX].size(1)), int(inp[K.LATTICE].size(0))
        nb_topo, nb_work = C.c_size_t(), C.c_size_t()
        _lib.check(lib.m3g_topology_bytes(N, E, T, S, C.byref(nb_topo)))
        topo = arena.take(nb_topo.value, fill, "topology")
        flags, hints = (C.c_int32 * 1)(0), C.c_int32(0)
        _lib.check(lib.m3g_topology_build_hints(N, E, T, S, p(inp[K.EDGE_INDEX]), p(inp[K.TRIPLET_EDGE_INDEX]), p(inp[K.BATCH]), p(topo),
                                                nb_topo.value, flags, C.byref(hints), M._stream()))
        torch.cuda.synchronize()
        assert flags[0] == 0, flags[0]
        arena.check()
        _lib.check(lib.m3g_workspace_bytes(eng.plan, N, E, T, S, C.byref(nb_work)))
        work = arena.take(nb_work.value, fill, "workspace")
        D, R, Cc, B = eng.cfg.embedding_dim, eng.cfg.n_max, eng.cfg.l_max * eng.cfg.n_max, eng.num_blocks
        shapes = {K.TOTAL_ENERGY: (S,)}
        if want_forces:
            shapes.update({K.FORCES: (N, 3), K.STRESSES: (S, 6)})
        shapes.update({K.SCALED_TOTAL_ENERGY: (S,), K.SCALED_ATOMIC_ENERGIES: (N,)})
        if extras:
            shapes.update({K.NODE_FEATURES: (N, D), K.EDGE_ATTR: (E, D), K.EDGE_DISTANCES: (E,), K.EDGE_WEIGHTS: (E, R), K.TRIPLET_ANGLES: (T,),
                           K.MID_EDGE_FEATURES: (B, E, Cc)})
        out = Outputs((key, arena.take_like(shape, torch.float32, fill, f"output {key}")) for key, shape in shapes.items())
        io = _lib.M3GIO(
            n_atoms=N, n_edges=E, n_triplets=T, n_structs=S, pos=p(inp[K.POS]), atom_types=p(inp[K.ATOM_TYPES]),
            edge_cell_shift=p(inp[K.EDGE_CELL_SHIFT]), lattice=p(inp[K.LATTICE]), topo=p(topo), triplet_edge_index=p(inp[K.TRIPLET_EDGE_INDEX]),
            total_energy=p(out[K.TOTAL_ENERGY]), forces=p(out.get(K.FORCES)), stresses=p(out.get(K.STRESSES)),
            scaled_total_energy=p(out[K.SCALED_TOTAL_ENERGY]), scaled_atomic_energies=p(out[K.SCALED_ATOMIC_ENERGIES]),
            node_features=p(out.get(K.NODE_FEATURES)), edge_attr=p(out.get(K.EDGE_ATTR)), edge_distances=p(out.get(K.EDGE_DISTANCES)),
            edge_weights=p(out.get(K.EDGE_WEIGHTS)), triplet_angles=p(out.get(K.TRIPLET_ANGLES)), mid_edge_features=p(out.get(K.MID_EDGE_FEATURES)),
            topo_hints=int(hints.value) if eng.topology_hints else 0)
        _lib.check(lib.m3g_energy_forces(eng.plan, C.byref(io), p(work), nb_work.value, M._stream()))
        torch.cuda.synchronize()
        arena.check()
        status = C.c_int32(0)
        _lib.check(lib.m3g_topology_status(N, E, T, S, p(topo), C.byref(status), M._stream()))
        assert status.value == 0, hex(status.value)
        arena.check()
        for key, t in inp.items():   # read-only means read-only
            assert _same_bits(t, originals[key]), key
    out.sizes = dict(N=N, E=E, T=T, S=S, workspace=nb_work.value, topology=nb_topo.value)
    return out


def _check_shape(shape, arch, sizes):
    """The regime the shape is in the table for, asserted on the lists the test runs on."""
    N, E, T, S = sizes
    want = SHAPES[shape][1]
    assert (N, S) == (want["N"], want["S"]), (shape, sizes)
    if shape in PART_FILLED:
        assert E % 16 != 0, (shape, E)
    if arch in (DEFAULT, DENSE):
        for key, got in (("E", E), ("T", T), ("e64", E % 64)):
            assert want.get(key, got) == got, (shape, key, got)
    if shape == "dense":
        assert T > 24 * E, (T, E)   # resolve_step_path: long_lists
    if shape == "fcc864":
        assert N % 16 == 0 and E % 16 == 0 and (E + 15) // 16 == 2268
    if shape == "lone":
        assert E == 0 and T == 0
    if shape == "pair":
        assert E == 2 and T == 0


def test_part_filled_tiles_of_the_shapes_on_the_host():
    """The residues the table claims, for every cutoff pair a shape is built with (no device work)."""
    e64 = set()
    for shape in SHAPES:
        arch = DENSE if shape == "dense" else DEFAULT
        sizes = _sizes(_host_batch(shape, arch[0], arch[1]))
        _check_shape(shape, arch, sizes)
        if shape in PART_FILLED:
            e64.add(sizes[1] % 64)
    assert len(e64) == len(PART_FILLED), e64
    for arch in (ANY_A, ANY_B):
        for shape in ANY_SIZE_SHAPES:
            _check_shape(shape, arch, _sizes(_host_batch(shape, arch[0], arch[1])))


@pytest.mark.parametrize("shape,selection", STEP_CASES)
def test_energy_forces_step_on_exact_size_buffers(shape, selection):
    K = _K()
    arch, precision, options, want_forces, extras = SELECTIONS[selection]
    arch = arch if arch is not None else DENSE if shape == "dense" else DEFAULT
    host = _host_batch(shape, arch[0], arch[1])
    _check_shape(shape, arch, _sizes(host))
    model = _model(arch)
    eng = model.engine
    moved = dict(options, precision=PRECISIONS[precision])
    try:
        eng.set_precision(precision)
        for name, value in options.items():
            eng.set_option(name, value)
        plain = model(host.clone().to(DEV), forces=want_forces, extras=extras)   # commits the plan; the result on torch's own buffers
        torch.cuda.synchronize()
        runs = [guarded_step(model, host.clone().to(DEV), fill, want_forces, extras) for fill in FILLS]
    finally:
        eng.set_precision("fp32")
        for name, value in DEFAULTS.items():
            if name != "precision" and (name in moved or (name == "small_tiles_fwd" and "small_tiles" in moved)):
                if not (name == "edge_kernel" and arch in (ANY_A, ANY_B)):   # (an any-size model takes no other value)
                    eng.set_option(name, value)
    zeros, ones = runs
    meta = zeros.sizes
    asked = [K.TOTAL_ENERGY, K.SCALED_TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES] + ([K.FORCES, K.STRESSES] if want_forces else []) + \
            ([K.NODE_FEATURES, K.EDGE_ATTR, K.EDGE_DISTANCES, K.EDGE_WEIGHTS, K.TRIPLET_ANGLES, K.MID_EDGE_FEATURES] if extras else [])
    assert sorted(zeros) == sorted(ones) == sorted(asked)
    for key in asked:
        if ones[key].numel() == 0:
            continue
        assert not bool(torch.isnan(ones[key]).any()), f"{key}: elements left holding the 0xFF fill (or computed from it)"
        assert _same_bits(zeros[key], ones[key]), f"{key}: depends on what the buffers held before the call"
        assert _same_bits(zeros[key], plain[key]), f"{key}: differs from the plain call"
    record_line(RECORD, f"{shape} {selection}: N {meta['N']} E {meta['E']} T {meta['T']} S {meta['S']} workspace {meta['workspace']} B "
                        f"topology {meta['topology']} B intact")


# ================================================================== 2. the capacity buffers of m3g_md_step
MD_BUFFERS = ("ei", "shift", "tei", "nti", "ntij", "pos32", "topo", "work")   # the order VerletGraph._md_prepare asks for them


def _md_walk(cells: int, fill, monkeypatch):
    """30 steps of VerletGraph.step of a `cells`^3 fcc Cu cell (default model, skin 0.3) along a fixed drift: atom i moves 0.006 A per
    step along a unit vector of its own.  Two atoms then come apart by at most 0.012 A per step, and the fcc shell nearest a cutoff
    is the one at 5.105 A, 0.105 A outside the two-body cutoff (three-body: 3.61 and 4.42 A about 4.0): step 1 cannot change a list
    (reuse), from step 9 on pairs may cross (refill), and past step 25 an atom has moved skin / 2 (a new search, inside `step`).
    `fill` None: torch's own buffers.  Returns (per-step outputs on the host, the final m3g_md_result.path of each step, the path of
    every m3g_md_step call, the buffers' sizes)."""
    from torch_m3gnet import _lib
    from torch_m3gnet.data import md
    from torch_m3gnet.data.md import VerletGraph

    K = _K()
    model = _model(DEFAULT)
    pos0, lat = _fcc(3.61, cells)
    arena, generation = Arena(DEV), itertools.count()
    names = itertools.cycle(MD_BUFFERS)

    def alloc(numel, dtype, device):
        name = next(names)
        gen = next(generation) // len(MD_BUFFERS)
        return arena.take_like((numel,), dtype, fill, f"{name} (set {gen})")

    lib = _lib.load_library()
    real_md_step, calls = lib.m3g_md_step, []

    def md_step(*args):   # every m3g_md_step call's m3g_md_result.path, kept (argument 7 is byref(result))
        rc = real_md_step(*args)
        calls.append(int(args[7]._obj.path))
        return rc

    with monkeypatch.context() as mp:
        if fill is not None:
            mp.setattr(md, "_alloc", alloc)
        mp.setattr(lib, "m3g_md_step", md_step)
        vg = VerletGraph([lat], [np.full(len(pos0), 29)], 5.0, 4.0, skin=0.3, device=DEV)
        drift = np.random.default_rng(21).normal(0.0, 1.0, pos0.shape)
        drift *= 0.006 / np.linalg.norm(drift, axis=1, keepdims=True)
        outs, paths = [], []
        for step in range(30):
            pos = pos0 + (step + 1) * drift
            out = vg.step(model, torch.tensor(pos, device=DEV))
            torch.cuda.synchronize()
            arena.check()
            vg.raise_on_step_errors(f"step {step}")
            paths.append(calls[-1])
            outs.append({key: out[key].cpu() for key in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)})
        sizes = {name: int(vg._md_buffers[name].numel() * vg._md_buffers[name].element_size()) for name in MD_BUFFERS}
    return outs, paths, calls, sizes


@pytest.mark.parametrize("cells,n_atoms", [(2, 32), (3, 108)])
def test_md_step_on_capacity_buffers_of_exact_size(cells, n_atoms, monkeypatch):
    from torch_m3gnet import _lib

    K = _K()
    plain, paths, all_paths, _ = _md_walk(cells, None, monkeypatch)
    assert len(plain[0][K.FORCES]) == n_atoms
    assert _lib.MD_UNSUPPORTED not in all_paths, all_paths
    assert set(paths) <= {_lib.MD_REUSE, _lib.MD_REFILL}, paths
    assert paths[0] == _lib.MD_REFILL and paths[1] == _lib.MD_REUSE and paths[2:].count(_lib.MD_REFILL) >= 1, paths   # (see _md_walk)
    for fill in FILLS:
        outs, fill_paths, fill_all, sizes = _md_walk(cells, fill, monkeypatch)
        assert fill_paths == paths and fill_all == all_paths, (fill, fill_paths, paths)
        for step, (got, want) in enumerate(zip(outs, plain)):
            for key in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES):
                assert not bool(torch.isnan(got[key]).any()), (fill, step, key)
                assert _same_bits(got[key], want[key]), (fill, step, key)
    record_line(RECORD, f"md_step fcc{n_atoms}: 30 steps, paths {''.join(map(str, paths))} (0 reuse, 1 refill; {all_paths.count(_lib.MD_NEED_SEARCH)} calls answered with a new search), capacity buffers "
                        + " ".join(f"{name} {nbytes} B" for name, nbytes in sizes.items()) + " intact")


# ================================================================== 3. the driver states
# Every driver asks `_driver.state_tensor` for its state, through the name its module imported: replaced here by one that asks the
# library for the size in the same way and answers with an arena buffer of exactly that size.  The kernels are driven through the
# kernel-level helpers of each driver's own test module (synthetic forces, no model), on the smallest batches that hold a one-row
# structure where the driver takes one, a structure of 257 rows (a full 256-row chunk + 1) and one in between.
def _state_seam(arena, fill, label):
    from torch_m3gnet import _lib

    def state_tensor(state_bytes, *sizes, device):
        nbytes = C.c_size_t()
        _lib.check(state_bytes(*sizes, C.byref(nbytes)))   # as _driver.state_tensor asks
        assert torch.device(device).type == "cuda"
        return arena.take(nbytes.value, fill, f"{label} state")

    return state_tensor


def _host(value):
    if isinstance(value, torch.Tensor):
        return value.detach().cpu().numpy()
    if isinstance(value, (tuple, list)) and value and isinstance(value[0], torch.Tensor):
        return np.stack([v.detach().cpu().numpy() for v in value])
    return np.asarray(value)


def _driver_on_guarded_states(monkeypatch, name, modules, run):
    """`run()` -> {what: tensor or array}: everything the driver's read() returns, its positions, cells and observables.  Three runs:
    torch's own state, then an arena state with 0x00 and with 0xFF inside; bands intact, everything bitwise equal."""
    results, sizes = {}, None
    for fill in (None,) + FILLS:
        arena = Arena(DEV)
        with monkeypatch.context() as mp:
            if fill is not None:
                for label, module in modules.items():
                    mp.setattr(module, "state_tensor", _state_seam(arena, fill, label))
            out = run()
            torch.cuda.synchronize()
            arena.check()
            results[fill] = {key: _host(val) for key, val in out.items()}
        if fill is not None:
            sizes = [(label, nbytes) for label, _, _, nbytes in arena._takes]
            assert {label for label, _ in sizes} == {f"{label} state" for label in modules}, sizes   # every seam was used
    plain = results[None]
    assert plain, name
    for fill in FILLS:
        assert sorted(results[fill]) == sorted(plain)
        for key, want in plain.items():
            assert _same_bits(results[fill][key], want), f"{name}: {key} depends on what the state held before init (fill {fill:#04x})"
    record_line(RECORD, f"driver {name}: " + ", ".join(f"{label} {nbytes} B" for label, nbytes in sizes) + " intact")


DRIVER_SIZES = [1, 40, 257]


def test_fire_state_on_exact_size_buffer(monkeypatch):
    import test_gpu_relax as t
    from torch_m3gnet import relax

    def run():
        st, out = t._run_kernel(DRIVER_SIZES, True, 10)
        return dict(out, pos=st.pos, lattice=st.lattice)

    _driver_on_guarded_states(monkeypatch, "FIRE", {"relax": relax}, run)


@functools.lru_cache(maxsize=None)
def _lbfgs_inputs(iters=10):
    """The chain's fp32 forces and stresses along the restatement's own trajectory, computed once (the same arrays for every run)."""
    import test_gpu_lbfgs as t

    chain = t.Chain(DRIVER_SIZES)
    refs = chain.references(True, memory=5)
    inputs = []
    for _ in range(iters):
        f, s = chain.forces(refs)
        inputs.append((f, s))
        for i, ref in enumerate(refs):
            a, b = chain.offs[i], chain.offs[i + 1]
            ref.step(f[a:b].astype(np.float64), s[i].astype(np.float64))
    return chain, inputs


def test_lbfgs_state_on_exact_size_buffer(monkeypatch):
    import test_gpu_lbfgs as t
    from torch_m3gnet import relax

    chain, inputs = _lbfgs_inputs()

    def run():
        st = t._state(chain.start, chain.lats, True, memory=5)   # 10 calls: the history of 5 pairs wraps
        for f, s in inputs:
            t._step(st, f, s)
        torch.cuda.synchronize()
        return dict(st.read(), pos=st.pos, lattice=st.lattice)

    _driver_on_guarded_states(monkeypatch, "L-BFGS", {"relax": relax}, run)


@pytest.mark.parametrize("ensemble", ["nvt_langevin", "npt_berendsen"])
def test_dyn_state_on_exact_size_buffer(ensemble, monkeypatch):
    import test_gpu_dynamics as t
    from torch_m3gnet import dynamics

    def run():
        st = t._state(ensemble, ensemble != "nvt_langevin", DRIVER_SIZES, temps=t.TEMPS[:3], seeds=t.SEEDS[:3])
        obs = t._run(st, DRIVER_SIZES, 10)
        return dict(st.read(), obs=obs, pos=st.pos, lattice=st.lattice)

    _driver_on_guarded_states(monkeypatch, f"dyn {ensemble}", {"dynamics": dynamics}, run)


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_mtk"])
def test_nhc_state_on_exact_size_buffer(ensemble, monkeypatch):
    import test_gpu_nhc as t
    from torch_m3gnet import dynamics

    sizes = [2, 40, 257]   # (tests/test_gpu_nhc.py starts at two atoms: one atom with a fixed centre of mass has no degree of freedom)

    def run():
        st = t._state(ensemble, True, sizes)
        obs, _ = t._run(st, sizes, 10)
        return dict(st.read(), obs=obs, pos=st.pos, lattice=st.lattice)

    _driver_on_guarded_states(monkeypatch, f"nhc {ensemble}", {"dynamics": dynamics}, run)


def test_remd_state_on_exact_size_buffer(monkeypatch):
    import remd_cases as rc
    import test_gpu_remd as t
    from torch_m3gnet import dynamics, replica_exchange

    def run():   # ladders of 2 x 257, 3 x 1 and 5 x 3 atoms through three rounds of step, step, exchange, step
        return t.Batch([0, 1, 2]).run(rc.schedule(3)).result()

    _driver_on_guarded_states(monkeypatch, "REMD", {"replica_exchange": replica_exchange, "dynamics": dynamics}, run)


def test_swap_mc_state_on_exact_size_buffer(monkeypatch):
    import test_gpu_mc as t
    from torch_m3gnet import monte_carlo

    def run():   # 2 (a swap needs two rows), 65 (masked) and 257 atoms, ten propose / decide rounds with forces and stresses
        return t.Batch([0, 3, 4], rounds=10).run().result()

    _driver_on_guarded_states(monkeypatch, "swap MC", {"monte_carlo": monte_carlo}, run)


def test_neb_state_on_exact_size_buffer(monkeypatch):
    import test_gpu_neb as t
    from torch_m3gnet import neb, relax

    def run():   # bands of 1 x 1, 1 x 257 and 3 x 32 interior image rows under FIRE
        st, fire, pos, snaps = t._run([(1, 1), (1, 257), (3, 32)], [11, 12, 13], 10)
        return dict(fire.read(), neb_forces=st.forces, neb_rows=st.rows, pos=pos, snaps=np.stack(snaps))

    _driver_on_guarded_states(monkeypatch, "NEB", {"neb": neb, "relax": relax}, run)


def test_phonon_state_on_exact_size_buffer(monkeypatch):
    import test_gpu_phonons as t
    from torch_m3gnet import phonons
    from torch_m3gnet.phonons import ph_displace, ph_dynamical_matrices, ph_force_constants

    structs = t._structures()   # 4, 1, 6 and 30 unit atoms: 2,592 / 144 / 432 / 360 displaced rows
    q = np.random.default_rng(7).uniform(-0.5, 0.5, (9, 3))

    def run():   # one displace / fit / sample cycle
        st = t._state(structs)
        out = dict(pos=ph_displace(st).clone())
        ph_force_constants(st, t._forces(st, 3), True)
        out.update(phi=st.phi, sums=st.sums, nonfinite=st.nonfinite)
        for s in range(len(structs)):
            out[f"d{s}"] = ph_dynamical_matrices(st, s, q)
        return out

    _driver_on_guarded_states(monkeypatch, "phonons", {"phonons": phonons}, run)


@pytest.mark.parametrize("kind", ["elastic", "eos"])
def test_elastic_state_on_exact_size_buffer(kind, monkeypatch):
    import elastic_reference as er
    import test_gpu_elastic as t
    from torch_m3gnet import elasticity
    from torch_m3gnet.elasticity import el_deform, el_fit_elastic, el_fit_eos

    rng = np.random.default_rng(5)
    lat257 = np.array([[15.0, 0.3, 0.0], [0.0, 14.5, 0.4], [0.2, -1.0, 16.0]])
    base = t._structures()
    structs = [base[1], (lat257, rng.uniform(0, 1, (257, 3)) @ lat257), base[4]]   # 1, 257 and 30 atoms
    deformations = t.ELASTIC if kind == "elastic" else er.eos_set([-0.07, -0.02, 0.013, 0.05, 0.11])

    def run():   # one deform / fit cycle
        st = t._state(structs, deformations)
        pos, lat = el_deform(st)
        out = dict(pos=pos.clone(), lat=lat.clone())
        if kind == "elastic":
            out.update(rows=el_fit_elastic(st, t._stresses(st, 1)), nonfinite=st.nonfinite)
        else:
            out.update(rows=el_fit_eos(st, t._energies(st, 2)), error=st.error)
        return out

    _driver_on_guarded_states(monkeypatch, f"elasticity {kind}", {"elasticity": elasticity}, run)


def test_trajectory_state_on_exact_size_buffer(monkeypatch):
    import test_gpu_trajectory as t
    from torch_m3gnet import trajectory

    def run():   # 1, 2, 3, 257 and 600 atoms; six samples (RDF, and MSD / VACF over 4 lags), every second one kicked
        return t._accumulate(6)

    _driver_on_guarded_states(monkeypatch, "trajectory", {"trajectory": trajectory}, run)
