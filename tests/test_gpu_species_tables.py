"""GPU: block 0's node rows from the per-species tables.  Block 0's x^0 is the species embedding, so x^0, v^0, TA^0 and TB^0 of an atom
depend on the committed weights and its species alone: the plan forms them once per species and precision at commit (k_node_pre_mfma
on num_types pseudo atoms) and a step copies them per atom beside the geometry stage (option species_tables = 1, the default;
StepPath::block0 in csrc/m3g_step_path.h).  Option 0 runs block 0's node kernel in every step, as before.

Everything here compares option 1 with option 0 in one process, bit for bit (the copy moves bits, and the tables are written by the
kernel, image and k order the step uses): energies, per-atom energies, forces, stresses, node features, final edge features and
mid_edge_features.  No tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from helpers import fcc_cu_graph, random_cell_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda"
# the large-system kernels on a small cell, the way tests/helpers.py forces them (small_tiles moves small_tiles_fwd with it; set anyway)
LARGE = dict(split_node_tiles=0, small_tiles=0, small_tiles_fwd=0)
DEFAULTS = dict(small_tiles=1536, small_tiles_fwd=3072, split_node_tiles=128, species_tables=1)   # an order that restores them
SELECTIONS = {"default": {}, "large": LARGE}


def _K():
    from torch_m3gnet.data import MaterialGraphKey as K

    return K


def _keys(forces=True):
    K = _K()
    return [K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR, K.MID_EDGE_FEATURES] + ([K.FORCES, K.STRESSES] if forces else [])


def _new_model(seed=0):
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(seed)
    model = build_model(cutoff=5.0, threebody_cutoff=4.0, l_max=3, n_max=3, num_types=95, embedding_dim=64, num_blocks=3)
    for m in model.model:   # documented chi so the three-body path (which reads v^0) carries weight
        if type(m).__name__ == "ThreeBodyInteration":
            m.nsb.factors = m.nsb.documented_factors()
    return model


@functools.lru_cache(maxsize=None)
def _model():
    """One model for the tests that change no weight; each puts the options it moved back."""
    return _new_model()


def _restore(model):
    model.engine.set_precision("fp32")
    for name, value in DEFAULTS.items():
        model.engine.set_option(name, value)
    model.engine.profile(False)


def _graph(cells):
    """Batch of [(lattice, positions, species)] at the default cutoffs."""
    from torch_m3gnet.data.material_graph import Batch, MaterialGraph

    return Batch.from_data_list([MaterialGraph.from_arrays(lat, pos, z, 5.0, 4.0) for lat, pos, z in cells]).to(DEV)


def _run(model, graph, tables, forces=True):
    model.engine.set_option("species_tables", tables)
    out = model(graph.clone(), forces=forces)
    torch.cuda.synchronize()
    return out, {k: out[k].clone() for k in _keys(forces)}


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32)   # (NaN == NaN, -0.0 != 0.0)


def _assert_same(on, off, what):
    assert on.keys() == off.keys()
    for k in on:
        assert on[k].shape == off[k].shape and torch.equal(_bits(on[k]), _bits(off[k])), (what, k)


def _launches(model, graph, tables):
    model.engine.set_option("species_tables", tables)
    return model.engine.count_launches(lambda: model(graph.clone(), extras=False))


def _compare(model, graph, what, forces=True):
    _, on = _run(model, graph, 1, forces)
    _, off = _run(model, graph, 0, forces)
    assert bool(torch.isfinite(on[_K().TOTAL_ENERGY]).all()), what
    _assert_same(on, off, what)
    return on


def test_cu32_default_selection_copies_beside_the_geometry_stage():
    """The small two-role launch: geometry stage + copy instead of geometry stage + k_node_pre_split's role; the same number of launches."""
    model, g = _model(), fcc_cu_graph(2, 2, 2).to(DEV)
    try:
        _compare(model, g, "cu32 default")
        assert _launches(model, g, 1) == _launches(model, g, 0)
    finally:
        _restore(model)


def test_cu32_large_system_kernels_one_launch_fewer():
    """The large two-role launch (any size): block 0's k_node_pre_mfma launch is gone, nothing else moves."""
    model, g = _model(), fcc_cu_graph(2, 2, 2).to(DEV)
    try:
        for name, value in LARGE.items():
            model.engine.set_option(name, value)
        _compare(model, g, "cu32 large")
        (k_on, o_on), (k_off, o_off) = _launches(model, g, 1), _launches(model, g, 0)
        assert k_on == k_off - 1 and o_on == o_off, (k_on, k_off, o_on, o_off)
    finally:
        _restore(model)


@pytest.mark.parametrize("forces", [True, False])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "f16x3"])
def test_random_species_cell_in_every_precision(precision, forces):
    """64 atoms of random species: each precision copies out of its own tables (its own image, and the f16x3 weight scale)."""
    model, g = _model(), _graph([random_cell_arrays(64, 9.1, seed=0)])
    assert len(set(g[_K().ATOM_TYPES].tolist())) > 30
    try:
        model.engine.set_precision(precision)
        for sel, options in SELECTIONS.items():
            for name, value in dict(DEFAULTS, **options).items():
                if name != "species_tables":
                    model.engine.set_option(name, value)
            _compare(model, g, f"n64 {precision} {sel}", forces)
    finally:
        _restore(model)


def test_batch_with_partial_tiles_and_the_ends_of_the_species_table():
    """5, 17 and 33 atoms: a structure smaller than a 16-atom tile, part-filled tiles, 55 atoms in all (the copy's last workgroup is
    part-filled too); species 0 and num_types - 1 are the first and the last row of every table."""
    cells = [list(random_cell_arrays(n, max(5.0, (14.0 * n) ** (1 / 3)), seed)) for seed, n in enumerate((5, 17, 33))]
    cells[0][2][0], cells[2][2][-1] = 1, 95   # atomic numbers: species index = Z - 1
    model, g = _model(), _graph(cells)
    types = g[_K().ATOM_TYPES].tolist()
    assert len(types) == 55 and 0 in types and 94 in types
    try:
        for sel, options in SELECTIONS.items():
            for name, value in options.items():
                model.engine.set_option(name, value)
            _compare(model, g, f"batch 5/17/33 {sel}")
    finally:
        _restore(model)


def test_tables_follow_every_commit_and_the_precision_of_the_call():
    """Stale tables: after a first call, an embedding row of a species in the cell and a first-layer weight of block 0's edge MLP
    change (in place: the engine commits again); the tables must be those of the new weights.  Then the precision changes with no
    commit in between: each precision's tables were formed at the last commit."""
    K = _K()
    model, g = _new_model(seed=1), _graph([random_cell_arrays(64, 9.1, seed=0)])
    params = dict(model.engine.seq.named_parameters())
    _, first = _run(model, g, 1)
    species = int(g[K.ATOM_TYPES][0])
    with torch.no_grad():
        params["3.linear.weight"][:, species] += 0.25                        # [D, num_types]: the species' embedding row
        params["7.concat_edge_update.dense.0.weight"][3, :64] += 0.125       # [D, 3 D]: columns of x_i, a TA^0 column
        params["6.linear_sigmoid1.weight"][1, :] -= 0.125                    # [C, D]: v^0
    after = _compare(model, g, "after the weights changed")
    assert not torch.equal(after[K.TOTAL_ENERGY], first[K.TOTAL_ENERGY]) and not torch.equal(after[K.FORCES], first[K.FORCES])
    for precision in ("bf16x3", "f16x3", "fp32"):
        model.engine.set_precision(precision)
        got = _compare(model, g, f"after the weights changed, then {precision}")
        if precision == "fp32":
            _assert_same(got, after, "back in fp32")


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_out_of_range_species_past_the_host_check(selection):
    """With the host's species check off: the copy clamps the index like the node kernel did (no table row outside [0, num_types)),
    the readout turns it into a NaN energy and the sticky M3G_TOPO_ERR_SPECIES bit -- the same bits as with option 0."""
    from torch_m3gnet.nn.modules import _Topology

    K = _K()
    model = _new_model()
    model.engine._check_species = lambda graph, probe: None
    for name, value in SELECTIONS[selection].items():
        model.engine.set_option(name, value)
    cells = [random_cell_arrays(12, 6.0, s) for s in range(3)]
    g = _graph(cells)
    for bad in (95, -3, 1 << 40):
        h = g.clone()
        types = h[K.ATOM_TYPES].clone()
        types[14] = bad              # an atom of the second structure
        h[K.ATOM_TYPES] = types
        out_on, on = _run(model, h, 1)
        status_on = _Topology.of(out_on).status()
        out_off, off = _run(model, h, 0)
        _assert_same(on, off, (selection, bad))
        e = on[K.TOTAL_ENERGY]
        assert bool(torch.isnan(e[1])) and bool(torch.isfinite(e[[0, 2]]).all()), (bad, e)
        assert status_on & 4 and _Topology.of(out_off).status() & 4


@pytest.mark.parametrize("blocks", [3, 1])
def test_last_blocks_edge_image_goes_unstored_when_nobody_reads_it(blocks):
    """The persistent exact-fp32 forward kernel with both layers saved skips the store of the last block's edge-feature image when
    the call has no edge_attr output (extras=False): its reverse kernels start from the saved activations.  A fresh model's first
    call is the one without the store (nothing of an earlier call in the workspace), then the same call with every optional output:
    energies, forces and stresses are the same bits.  One block: the first block (it forms e0 itself) is the last one too."""
    from torch_m3gnet.model.build import build_model

    K = _K()
    torch.manual_seed(2)
    model = build_model(cutoff=5.0, threebody_cutoff=4.0, l_max=3, n_max=3, num_types=95, embedding_dim=64, num_blocks=blocks)
    for name, value in LARGE.items():
        model.engine.set_option(name, value)
    g = fcc_cu_graph(2, 2, 2).to(DEV)
    lean = model(g.clone(), forces=True, extras=False)
    torch.cuda.synchronize()
    lean = {k: lean[k].clone() for k in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)}
    full = model(g.clone(), forces=True, extras=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(full[K.EDGE_ATTR]).all()) and float(full[K.EDGE_ATTR].abs().max()) > 0
    for k, v in lean.items():
        assert torch.equal(_bits(v), _bits(full[k])), k


def test_copy_as_a_launch_of_its_own_without_edges_and_under_the_stage_profiler():
    """StepPath::block0 = a launch of its own: a lone atom (no edge, so no geometry launch; the readout still reads x^0) and a pair
    (no triplet), and any cell with the stage profiler on, where the copy is timed as the node_pre stage of block 0."""
    model = _model()
    lone = (np.eye(3) * 20.0, np.array([[10.0, 10.0, 10.0]]), np.array([29]))
    pair = (np.eye(3) * 20.0, np.array([[10.0, 10.0, 10.0], [13.0, 10.0, 10.0]]), np.array([29, 8]))
    try:
        _compare(model, _graph([lone]), "lone atom")
        _compare(model, _graph([pair, lone]), "pair + lone atom")
        g = fcc_cu_graph(2, 2, 2).to(DEV)
        plain = _compare(model, g, "cu32")
        model.engine.profile(True)
        stages = {}
        for tables in (1, 0):
            _, out = _run(model, g, tables)
            _assert_same(out, plain, f"cu32 profiled, species_tables {tables}")
            stages[tables] = model.engine.profile_read()
        assert stages[1]["node_pre"][1] == stages[0]["node_pre"][1] == 3 and stages[1]["geometry_basis"][1] == 1, stages
    finally:
        _restore(model)
