"""The persistent (large-system) kernels against the fp64 oracle on every kind of parity input.

The default selection (resolve_step_path, csrc/m3g_step_path.h) sends cells of up to 1,536 edge tiles / 128 atom tiles down the
small-system path and takes a workgroup's single left-over tile out of the queue of k_edge_rev_f32, so on the fixtures, the
hyper-parameter sweep and the fuzz none of the kernels the headline number is timed on runs.  Here they are forced
(helpers.PERSISTENT: small_tiles = 0 -> k_edge_block_mfma<TBS, fp32, SAVE> + k_edge_rev_f32<TBS, NEED_DP1, 8, SAVED_P2>,
split_node_tiles = 0 -> k_node_pre_mfma<fp32> + k_readout_mfma<fp32>, split_tail = 0 -> every tile through the whole-tile body)
on the fixtures, on the model shapes TBS = 1, 2, 3, 4 / padded widths / n_max = 4, with the kernel pair (rev_kernel = 0), in the
f16x3 and bf16x3 modes, and on an 864-atom cell where a wave of the reverse kernel takes a second tile.  Every test that claims a
regime of the tile queue asserts it on its own input with helpers.persistent_tile_counts (pinned to the kernels' code by
tests/test_step_path_cpu.py).

Gates (BASELINE.json north_star, tests/test_gpu_parity.py): E 1e-5, F and stresses 1e-4 of their largest component,
mid_edge_features 1e-4 per block, x and edge_attr 1e-5; bf16x3: E 1e-3, F 5e-4, stresses 2e-3 (test_saturated_activations_stress_case).
Measured margins: profiles/persistent_path_margins.txt.  Reference behaviour: nn/gradient.py:25-64, nn/conv.py:63-97."""
import functools

import numpy as np
import pytest
import torch

from helpers import (CASES, PERSISTENT, PERSISTENT_TAIL, build_engine_model, engine_graph, fcc_cu_graph, load_oracle_case,
                     persistent_tile_counts, random_cell_graph, record_line, rel_err, set_options, split_tail_runs,
                     wave_takes_a_second_tile)
from oracle import m3gnet_oracle as orc
from test_gpu_properties import _oracle_inputs

pytestmark = pytest.mark.gpu

MARGINS = "persistent_path_margins.txt"
GATES = {"fp32": dict(e=1e-5, f=1e-4, s=1e-4), "f16x3": dict(e=1e-5, f=1e-4, s=1e-4), "bf16x3": dict(e=1e-3, f=5e-4, s=2e-3)}


def _keys():
    from torch_m3gnet.data import MaterialGraphKey as K

    forward = (K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR, K.MID_EDGE_FEATURES)
    return K, forward, forward + (K.FORCES, K.STRESSES)


def _outputs(model, graph):
    _, _, keys = _keys()
    g = model(graph)
    torch.cuda.synchronize()
    return {k: g[k].clone() for k in keys}


def _oracle64(model, graph):
    """fp64 evaluation of the oracle with the exact derivative on the model's own weights and constants."""
    torch.set_num_threads(8)
    p, cfg, c, og = _oracle_inputs(model, graph)
    p64 = {k: v.double() for k, v in p.items()}
    c64 = orc.make_constants(cfg, c.elemental_energies, dtype=torch.float64)   # constants formed in fp64, as the sweep's oracle call does
    c64.factors = c.factors.double()
    return orc.energy_forces(p64, cfg, c64, og, legendre_backward="exact"), cfg


def _errors(out, o, blocks):
    K, _, _ = _keys()
    e = float(((out[K.TOTAL_ENERGY].double().cpu() - o["total_energy"]).abs() / o["total_energy"].abs()).max())
    return dict(e=e, f=rel_err(out[K.FORCES], o["forces"]), s=rel_err(out[K.STRESSES], o["stresses"]),
                x=rel_err(out[K.NODE_FEATURES], o["x"]), ea=rel_err(out[K.EDGE_ATTR], o["edge_attr"]),
                m=max(rel_err(out[K.MID_EDGE_FEATURES][b], o[f"mid_edge_features_{b}"]) for b in range(blocks)))


def _fmt(err):
    return "E %.2e  F %.2e  stress %.2e  x %.2e  edge_attr %.2e  mid_edge_features %.2e" % tuple(err[k] for k in ("e", "f", "s", "x", "ea", "m"))


def _two_selections(a, b):
    """Forward outputs bit-identical between two kernel selections of the fp32 mode; returns how far forces and stresses are apart."""
    K, forward, _ = _keys()
    for k in forward:
        assert torch.equal(a[k], b[k]), k
    return rel_err(a[K.FORCES], b[K.FORCES]), rel_err(a[K.STRESSES], b[K.STRESSES])


# ------------------------------------------------------------------ 1. the fixtures
@pytest.mark.parametrize("case,mode", CASES)
def test_persistent_kernels_on_the_fixtures(case, mode):
    """Every fixture (fitted, triclinic, mixed-scale, 6 - 130 atoms; at most 256 tiles, so every workgroup has one tile or none) in
    fp32 under PERSISTENT: against the fp64 oracle at the gates of test_engine_vs_golden_and_oracle, and against the default
    selection -- forward outputs bit for bit, forces and stresses within 1e-5 and NOT equal: the whole-tile body of k_edge_rev_f32
    associates dL/dh and dL/dm differently from the split-tile kernel, so equal forces would mean it never ran."""
    K, _, _ = _keys()
    _, cfg, _, graph, _ = load_oracle_case(case, mode)
    counts = persistent_tile_counts(graph["edge_index"].shape[1])
    assert max(counts) == 1, counts   # the regime: one whole tile per workgroup, which split_tail = 1 would take out of the queue
    model, _ = build_engine_model(case, mode)
    default = _outputs(model, engine_graph(graph))
    out = _outputs(set_options(model, **PERSISTENT), engine_graph(graph))
    p64, cfg64, c64, graph64, _ = load_oracle_case(case, mode, dtype=torch.float64)
    o = orc.energy_forces(p64, cfg64, c64, graph64, legendre_backward="exact")
    err = _errors(out, o, cfg.num_blocks)
    f_diff, s_diff = _two_selections(default, out)
    record_line(MARGINS, f"fixture {case}_{mode} fp32 persistent vs fp64 oracle: {_fmt(err)};  vs default selection: forward bit-identical, "
                         f"F {f_diff:.2e}  stress {s_diff:.2e}")
    assert err["e"] < 1e-5 and err["f"] < 1e-4 and err["s"] < 1e-4, err
    assert err["x"] < 1e-5 and err["ea"] < 1e-5, err
    if case != "alna":   # alna's neighbours sit on the three-body cutoff: m is ~1e-17, pure rounding
        assert err["m"] < 1e-4, err
    assert 0.0 < f_diff < 1e-5 and s_diff < 1e-5, (f_diff, s_diff)


# ------------------------------------------------------------------ 2. model shapes
# the five MFMA rows of test_hyperparameter_sweep_against_oracle (tests/test_gpu_properties.py) on that test's own three cells
SHAPES = [(1, 1, 8, 1, 4.0, 3.0),     # C = 1: TBS = 1, width 8 padded to 64
          (2, 2, 33, 4, 4.5, 4.5),    # C = 4: TBS = 1, odd width, 4 blocks
          (4, 4, 64, 2, 5.0, 3.5),    # C = 16: TBS = 4 (list kernels: l_max = 4)
          (3, 4, 48, 1, 4.2, 4.0),    # C = 12: TBS = 3, n_max = 4 layout of the node tables
          (4, 1, 16, 3, 5.0, 4.0)]    # C = 4: TBS = 1
SELECTIONS = {"persistent": ("fp32", PERSISTENT), "persistent_pair": ("fp32", dict(PERSISTENT, rev_kernel=0)),
              "f16x3": ("f16x3", {}), "bf16x3": ("bf16x3", {})}


def _sweep_model(l_max, n_max, dim, blocks, cut, tb_cut, elemental=(-1.0, 1.0)):
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(11)
    model = build_model(cut, tb_cut, l_max, n_max, 60, dim, blocks, elemental_energies=torch.linspace(*elemental, 60), energy_scale=1.7)
    for m in model.model:
        if type(m).__name__ == "ThreeBodyInteration":
            m.nsb.factors = m.nsb.documented_factors()
    return model


def _sweep_batch(cut, tb_cut):
    from torch_m3gnet.data.material_graph import Batch

    return Batch.from_data_list([random_cell_graph(14 + 3 * s, 6.0 + 0.3 * s, 20 + s, cutoff=cut, tb_cutoff=tb_cut, zmax=59) for s in range(3)])


@functools.lru_cache(maxsize=None)
def _sweep_oracle(row):
    """One fp64 oracle evaluation per row, shared by the four selections (never modified)."""
    return _oracle64(_sweep_model(*SHAPES[row]), _sweep_batch(*SHAPES[row][4:]))[0]


@pytest.mark.parametrize("selection", list(SELECTIONS))
@pytest.mark.parametrize("row", range(len(SHAPES)))
def test_model_shapes_on_the_persistent_kernels_and_in_every_mode(row, selection):
    """C = 1, 4, 12, 16 (TBS = 1, 3, 4 of k_edge_block_mfma / k_edge_rev_f32; TBS = 2 is in the fuzz and the trained-like test below),
    widths 8 - 64, 1 - 4 blocks: fp32 on the persistent kernels, fp32 on the persistent forward kernel + the reverse kernel pair,
    and the f16x3 / bf16x3 modes (whose kernels are the persistent ones at every size) against the fp64 oracle."""
    l_max, n_max, dim, blocks, cut, tb_cut = SHAPES[row]
    precision, options = SELECTIONS[selection]
    model = _sweep_model(*SHAPES[row])
    model.engine.set_precision(precision)
    out = _outputs(set_options(model, **options), _sweep_batch(cut, tb_cut).to("cuda"))
    err = _errors(out, _sweep_oracle(row), blocks)
    record_line(MARGINS, f"shape l_max {l_max} n_max {n_max} width {dim} blocks {blocks}, {selection}: {_fmt(err)}")
    gate = GATES[precision]
    assert err["e"] < gate["e"] and err["f"] < gate["f"] and err["s"] < gate["s"], err
    if precision != "bf16x3":
        assert err["ea"] < 1e-5 and err["m"] < 1e-4, err


# ---- the same chains where the three-body pre-activations carry weight
# Random-init weights keep W m of the three-body gated update near zero, where SiLU' and the sigmoid barely move: a wrong k-step of
# the TBS chain (tb_preact) changes the forces of the rows above by less than their gates (tried: step 3 of TBS = 4 reading step 2's
# channels passes them).  With weights x 4 and biases x 2 (tests/test_gpu_parity.py, _scaled_like_trained) it does not.  One row per
# TBS; reference arithmetic on these inputs (fp32 CPU oracle against the fp64 oracle): within E 5.4e-7, F 2.6e-6, stress 2.8e-6,
# mid_edge_features 3.0e-6 -- 18 x or more inside the gates.
TRAINED_LIKE_SHAPES = [(2, 2), (2, 4), (3, 4), (4, 4)]   # (l_max, n_max): C = 4, 8, 12, 16 -> TBS = 1, 2, 3, 4


def _trained_like_model(l_max, n_max):
    # (elemental energies of one sign: with the sweep's -1 .. 1 the totals of these cells are remainders of cancelling terms, and the
    #  fp32 reference itself misses the 1e-5 energy gate)
    model = _sweep_model(l_max, n_max, 64, 2, 5.0, 4.0, elemental=(-3.0, -1.0))
    with torch.no_grad():
        for name, p in model.model.named_parameters():
            p.mul_(2.0 if name.endswith("bias") else 4.0)
    return model


@pytest.mark.parametrize("l_max,n_max", TRAINED_LIKE_SHAPES)
def test_three_body_chain_steps_with_trained_like_weights(l_max, n_max):
    """TBS = 1, 2, 3, 4 of k_edge_block_mfma<fp32> / k_edge_rev_f32 (PERSISTENT) and of the split-tile kernels (default selection) on
    the sweep's cells with weights scaled like a trained potential's: both against the fp64 oracle, and against each other (forward
    bit for bit, forces and stresses within 1e-5 and not equal)."""
    model = _trained_like_model(l_max, n_max)
    batch = _sweep_batch(5.0, 4.0)
    o, _ = _oracle64(model, batch)
    default = _outputs(model, batch.clone().to("cuda"))
    out = _outputs(set_options(model, **PERSISTENT), batch.clone().to("cuda"))
    f_diff, s_diff = _two_selections(default, out)
    for name, res in (("persistent", out), ("default selection", default)):
        err = _errors(res, o, 2)
        record_line(MARGINS, f"trained-like weights, l_max {l_max} n_max {n_max} width 64 blocks 2, {name}: {_fmt(err)}"
                             + (f";  persistent vs default selection: F {f_diff:.2e}  stress {s_diff:.2e}" if res is out else ""))
        # (edge_attr is recorded, not gated: the fp32 reference itself sits 1.6e-6 .. 2.8e-6 from fp64 on these inputs, under 4 x inside 1e-5)
        assert err["e"] < 1e-5 and err["f"] < 1e-4 and err["s"] < 1e-4 and err["m"] < 1e-4, (name, err)
    assert 0.0 < f_diff < 1e-5 and s_diff < 1e-5, (f_diff, s_diff)


# ------------------------------------------------------------------ 4. a second tile per wave, outside the default architecture
# 6 x 6 x 6 fcc cell (864 atoms), species 1..59 at random, cutoff 5.0.  jitter 0.1: 37,380 edges, 10 tiles per workgroup (a wave of
# k_edge_rev_f32 comes round its loop again: prefetched nci hand-over, has_next; no left-over tile for split_tail = 1); jitter 0.06:
# 36,450 edges, 9 tiles per workgroup = 8 whole + 1 through the split tail.
# Reference arithmetic on these inputs (fp32 CPU oracle against the fp64 oracle, checked on the CPU for all four rows): jitter 0.1
# within E 8.7e-7, F 4.1e-6, stress 6.8e-6, mid_edge_features 9.0e-6; jitter 0.06 within E 9.2e-7, F 6.1e-6, stress 4.8e-6,
# mid_edge_features 6.0e-6 -- everywhere more than 10 x inside the gates below.  (The bench's own jitter 0.025 leaves forces that are
# the remainder of cancelling terms, max|F| ~ 1e-3: the fp32 reference itself is then 1.1e-5 / 1.3e-5 off on F / stress, less than
# 10 x inside, so it is not used.)
SECOND_TILE_SHAPES = [(1, 1, 8, 1, 3.5), (4, 4, 64, 2, 3.5), (3, 4, 48, 1, 4.0), (2, 2, 33, 4, 4.0)]   # TBS = 1, 4, 3, 1


def _species_cell(jitter, tb_cut):
    from torch_m3gnet.data.material_graph import Batch, MaterialGraph
    from torch_m3gnet.data.synthetic import fcc_cu_arrays

    lat, pos, _ = fcc_cu_arrays(6, 6, 6, jitter=jitter)
    z = np.random.default_rng(2).integers(1, 60, len(pos))
    return Batch.from_data_list([MaterialGraph.from_arrays(lat, pos, z, 5.0, tb_cut)])


@pytest.mark.parametrize("l_max,n_max,dim,blocks,tb_cut", SECOND_TILE_SHAPES)
def test_second_tile_per_wave_and_split_tail_outside_the_default_architecture(l_max, n_max, dim, blocks, tb_cut):
    K, _, _ = _keys()
    shape = (l_max, n_max, dim, blocks, 5.0, tb_cut)
    # ---- a wave's second tile: every tile whole
    cell = _species_cell(0.1, tb_cut)
    counts = persistent_tile_counts(int(cell[K.NUM_EDGES]))
    assert int(cell[K.NUM_NODES]) == 864 and wave_takes_a_second_tile(counts) and not split_tail_runs(counts, 1), counts
    model = _sweep_model(*shape)
    out = _outputs(set_options(model, **PERSISTENT), cell.clone().to("cuda"))
    err = _errors(out, _oracle64(model, cell)[0], blocks)
    record_line(MARGINS, f"864 atoms, {int(cell[K.NUM_EDGES])} edges, tiles per workgroup {dict(counts)}, l_max {l_max} n_max {n_max} width {dim} "
                         f"blocks {blocks}, persistent, every tile whole: {_fmt(err)}")
    assert err["e"] < 1e-5 and err["f"] < 1e-4 and err["s"] < 1e-4 and err["m"] < 1e-4, err
    # ---- whole tiles, then the split tail (rev_split_run inside k_edge_rev_f32<TBS>)
    cell = _species_cell(0.06, tb_cut)
    counts = persistent_tile_counts(int(cell[K.NUM_EDGES]))
    assert wave_takes_a_second_tile(counts) and split_tail_runs(counts, 1), counts
    model = _sweep_model(*shape)
    tail = _outputs(set_options(model, **PERSISTENT_TAIL), cell.clone().to("cuda"))
    whole = _outputs(set_options(model, **PERSISTENT), cell.clone().to("cuda"))
    err = _errors(tail, _oracle64(model, cell)[0], blocks)
    f_diff, s_diff = _two_selections(tail, whole)
    record_line(MARGINS, f"864 atoms, {int(cell[K.NUM_EDGES])} edges, tiles per workgroup {dict(counts)}, l_max {l_max} n_max {n_max} width {dim} "
                         f"blocks {blocks}, persistent + split tail: {_fmt(err)};  vs every tile whole: F {f_diff:.2e}  stress {s_diff:.2e}")
    assert err["e"] < 1e-5 and err["f"] < 1e-4 and err["s"] < 1e-4 and err["m"] < 1e-4, err
    assert 0.0 < f_diff < 1e-5 and s_diff < 1e-5, (f_diff, s_diff)   # (> 0: the tail really ran)


# ------------------------------------------------------------------ 5. the restatement of the tile queue against the device
# (cells, split_tail settings that must give the bits of split_tail = 0, settings that must not)
TAIL_REGIMES = [((3, 3, 3), (1,), (2,)),     # 108 atoms, 284 tiles: 2 per workgroup -- nothing for split_tail = 1, both tiles for 2
                ((6, 6, 6), (), (1,)),       # 864 atoms, 2,268 tiles: 9 / 5 / 1 per workgroup
                ((4, 4, 4), (1, 2), ())]     # 256 atoms, 672 tiles: 3 per workgroup -- no tail under either setting


@pytest.mark.parametrize("cells,same,different", TAIL_REGIMES)
def test_split_tail_runs_exactly_where_the_restated_queue_says(cells, same, different):
    """helpers.persistent_tile_counts says which workgroups have a left-over tile; the device agrees: where it says none, split_tail
    changes no bit of the forces, where it says some, the forces move (by less than 1e-5) -- with the LJ-fitted model, and every
    setting against the fp64 oracle."""
    K, _, _ = _keys()
    g0 = fcc_cu_graph(*cells)
    counts = persistent_tile_counts(int(g0[K.NUM_EDGES]))
    for mode in same:
        assert not split_tail_runs(counts, mode), (counts, mode)
    for mode in different:
        assert split_tail_runs(counts, mode), (counts, mode)
    model, cfg = build_engine_model("cu32fit", "doc")
    whole = _outputs(set_options(model, **PERSISTENT), g0.clone().to("cuda"))
    o, _ = _oracle64(model, g0)
    for mode in (0,) + same + different:
        out = whole if mode == 0 else _outputs(set_options(model, split_tail=mode), g0.clone().to("cuda"))
        err = _errors(out, o, cfg.num_blocks)
        f_diff, s_diff = _two_selections(out, whole)
        record_line(MARGINS, f"{int(g0[K.NUM_NODES])} atoms, tiles per workgroup {dict(counts)}, fitted model, split_tail {mode}: {_fmt(err)};  "
                             f"vs split_tail 0: F {f_diff:.2e}  stress {s_diff:.2e}")
        assert err["e"] < 1e-5 and err["f"] < 1e-4 and err["s"] < 1e-4 and err["m"] < 1e-4, (mode, err)
        if mode in same:
            assert torch.equal(out[K.FORCES], whole[K.FORCES]) and torch.equal(out[K.STRESSES], whole[K.STRESSES]), mode
        elif mode in different:
            assert 0.0 < f_diff < 1e-5 and s_diff < 1e-5, (mode, f_diff, s_diff)
