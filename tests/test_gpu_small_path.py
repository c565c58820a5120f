"""The small-system path (plan option "small_tiles"; csrc/m3g_edge_small.hip and the fused tail launches) against the
large-system kernels on the same inputs, and the large-system kernels against the reference's numbers on the fixtures (which
the default selection now sends down the small path).

Contract: every dense chain of the split-tile edge kernels is the same k-ordered fp32 fmaf chain the persistent
kernels form, so energies, per-atom energies, node / edge features and the three-body aggregates are BIT-IDENTICAL between
the two paths; forces and stresses agree to 1e-5 of their largest component ("large path" means the whole-tile body of the
persistent reverse kernel: _run switches option split_tail off with the split-tile kernels, or a fixture's one tile per
workgroup would go to the split body again; two sums of the reverse pass -- dL/dh of an edge and dL/dm -- are associated per
wave, in a fixed order; measured differences 8.7e-8 .. 1.8e-6 on the forces, 8.1e-8 .. 6.2e-6 on the stresses, never zero, the
largest on the random-init cu32 cells whose forces are sums of cancelling terms -- the fp32 path itself sits 1.3e-5 from the fp64 oracle
there; gpurun_out/small_vs_large_margins.txt).  Reference behaviour: nn/gradient.py:25-64 on the small cells
of tests/conftest.py:89-115."""
import pytest
import torch

from helpers import CASES, build_engine_model, engine_graph, load_oracle_case, rel_err

pytestmark = pytest.mark.gpu

SMALL_CASES = [("cu32", "doc"), ("cu32", "ref"), ("tio", "doc"), ("mix", "doc"), ("tri", "doc"), ("cu32fit", "doc"), ("mixfit", "doc"),
               ("alna", "ref"), ("cu32pair", "doc")]


def _run(case, mode, small_tiles, forces=True):
    from torch_m3gnet.data import MaterialGraphKey as K

    model, _ = build_engine_model(case, mode)
    model.engine.set_option("small_tiles", small_tiles)
    if small_tiles == 0:
        # a fixture has at most 256 tiles: one per workgroup, which split_tail = 1 would take out of the queue of k_edge_rev_f32 and
        # hand to rev_split_run, the split-tile kernel's own body -- the "large path" would be the small one again
        model.engine.set_option("split_tail", 0)
    _, _, _, graph, expect = load_oracle_case(case, mode)
    g = model(engine_graph(graph), forces=forces)
    torch.cuda.synchronize()
    keys = [K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR, K.MID_EDGE_FEATURES]
    if forces:
        keys += [K.FORCES, K.STRESSES]
    return {k: g[k].clone() for k in keys}, expect


@pytest.mark.parametrize("case,mode", SMALL_CASES)
def test_small_path_equals_large_path(case, mode):
    from torch_m3gnet.data import MaterialGraphKey as K

    small, _ = _run(case, mode, 1 << 20)
    large, _ = _run(case, mode, 0)
    for k in (K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR, K.MID_EDGE_FEATURES):
        assert torch.equal(small[k], large[k]), k
    f_err, s_err = rel_err(small[K.FORCES], large[K.FORCES]), rel_err(small[K.STRESSES], large[K.STRESSES])
    import os
    if os.path.isdir("gpurun_out"):
        with open("gpurun_out/small_vs_large_margins.txt", "a") as fh:
            fh.write(f"{case}_{mode}: forward outputs bit-identical; F {f_err:.2e} of max|F| = {float(large[K.FORCES].abs().max()):.3e}, stress {s_err:.2e}\n")
    assert 0.0 < f_err < 1e-5   # (> 0: the whole-tile body of k_edge_rev_f32 associates dL/dh and dL/dm differently -- it really ran)
    assert s_err < 1e-5


@pytest.mark.parametrize("case,mode", [("cu32", "doc"), ("mix", "doc")])
def test_small_path_energy_only_call(case, mode):
    """forces=False: nothing is saved for a reverse pass (SAVE = 0 instantiation); same energies, bit for bit."""
    from torch_m3gnet.data import MaterialGraphKey as K

    small, _ = _run(case, mode, 1 << 20, forces=False)
    large, _ = _run(case, mode, 0, forces=False)
    full, _ = _run(case, mode, 1 << 20, forces=True)
    for k in (K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR):
        assert torch.equal(small[k], large[k]), k
        assert torch.equal(small[k], full[k]), k


@pytest.mark.parametrize("case,mode", CASES)
def test_large_path_on_the_fixtures(case, mode):
    """The persistent kernels (small_tiles = 0) against the reference's own numbers: the default selection no longer runs them on
    cells this small, the 10,000-atom tests and this one keep them pinned."""
    from torch_m3gnet.data import MaterialGraphKey as K

    g, expect = _run(case, mode, 0)
    assert rel_err(g[K.NODE_FEATURES], expect["out_x"]) < 1e-5
    assert rel_err(g[K.EDGE_ATTR], expect["out_edge_attr"]) < 1e-5
    e_ref = expect["out_total_energy"]
    assert float(((g[K.TOTAL_ENERGY].cpu() - e_ref).abs() / e_ref.abs()).max()) < 1e-5
    # (doc mode: the reference's own forces carry its Legendre-backward defect, tests/test_gpu_parity.py; the gate there is the
    #  exact fp64 derivative -- here the two paths are tied to each other at 1e-5 above, and this path to the reference loosely)
    assert rel_err(g[K.FORCES], expect["out_forces"]) < (1e-4 if mode == "ref" else 5e-3)


def test_small_path_is_deterministic_and_selected_by_size():
    """25 repeats of the 32-atom cell through the split-tile kernels: identical bits every time; and a threshold below the
    cell's tile count selects the persistent kernels (same energies bit for bit, see above)."""
    from torch_m3gnet.data import MaterialGraphKey as K

    model, _ = build_engine_model("cu32fit", "doc")
    _, _, _, graph, _ = load_oracle_case("cu32fit", "doc")
    g0 = model(engine_graph(graph))
    ref = {k: g0[k].clone() for k in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)}
    for _ in range(25):
        g = model(engine_graph(graph))
        for k, v in ref.items():
            assert torch.equal(g[k], v), k
    tiles = (graph["edge_index"].shape[1] + 15) // 16
    model.engine.set_option("small_tiles", tiles - 1)   # one tile too many for the small path
    g = model(engine_graph(graph))
    assert torch.equal(g[K.TOTAL_ENERGY], ref[K.TOTAL_ENERGY])
    assert rel_err(g[K.FORCES], ref[K.FORCES]) < 1e-5


@pytest.mark.parametrize("case,mode", [("cu32", "doc"), ("mix", "doc"), ("tri", "doc"), ("mixfit", "doc"), ("alna", "ref")])
def test_fused_launches_are_bit_identical(case, mode):
    """Option small_launches: the fused launches (readout + per-structure energy sums; geometry reverse + force gather + virial)
    form every sum in the order of the kernels they replace -- energies, forces and stresses equal bit for bit."""
    from torch_m3gnet.data import MaterialGraphKey as K

    outs = []
    for fused in (1, 0):
        model, _ = build_engine_model(case, mode)
        model.engine.set_option("small_launches", fused)
        _, _, _, graph, _ = load_oracle_case(case, mode)
        g = model(engine_graph(graph))
        outs.append({k: g[k].clone() for k in (K.TOTAL_ENERGY, K.SCALED_TOTAL_ENERGY, K.FORCES, K.STRESSES)})
    for k, v in outs[0].items():
        assert torch.equal(v, outs[1][k]), k


def test_fused_launches_on_a_larger_cell_and_many_structures():
    """864-atom cell (force gather ends with the virial; readout with the energy sum), a 2,048-atom cell (beyond the fused sums' range:
    the energy sums are deferred into the final stress launch) and a 12-structure batch (more structures than the fused launches
    walk: the stand-alone sum kernels run) -- identical bits with and without the option."""
    from helpers import fcc_cu_graph, random_cell_graph
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.material_graph import Batch

    graphs = [fcc_cu_graph(6, 6, 6).to("cuda"), fcc_cu_graph(8, 8, 8).to("cuda"),
              Batch.from_data_list([random_cell_graph(12, 6.0, s) for s in range(12)]).to("cuda")]
    for g0 in graphs:
        outs = []
        for fused in (1, 0):
            model, _ = build_engine_model("cu32", "doc")
            model.engine.set_option("small_launches", fused)
            g = model(g0.clone())
            outs.append({k: g[k].clone() for k in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)})
        for k, v in outs[0].items():
            assert torch.equal(v, outs[1][k]), k


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "bf16x3"])
def test_node_and_threebody_reverse_in_one_launch_is_bit_identical(precision):
    """Option fuse_node_tb: the three-body reverse (moment path) and the node reverse of a block run as two workgroup roles of one
    launch (k_node_tb_reverse; the node role's v-gradient term waits for the three-body role's rows inside the launch and is then
    gathered in the one-pass order).  Same bits as the two launches, on fixtures and on a 108-atom cell, in every mode."""
    from helpers import fcc_cu_graph
    from torch_m3gnet.data import MaterialGraphKey as K

    # (the launch is taken for cells of at most 128 atoms -- beyond that its in-launch publishing costs more than a launch boundary;
    #  the 108-atom cell is the largest fcc cell below the limit)
    cases = [engine_graph(load_oracle_case(c, m)[3]) for c, m in (("cu32fit", "doc"), ("mixfit", "doc"), ("tri", "doc"))] + [fcc_cu_graph(3, 3, 3).to("cuda")]
    names = [("cu32fit", "doc"), ("mixfit", "doc"), ("tri", "doc"), ("cu32fit", "doc")]
    for g0, (c, m) in zip(cases, names):
        outs = []
        for fused in (1, 0):
            model, _ = build_engine_model(c, m)
            model.engine.set_precision(precision)
            model.engine.set_option("fuse_node_tb", fused)
            g = model(g0.clone() if hasattr(g0, "clone") else g0)
            outs.append({k: g[k].clone() for k in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)})
        for k, v in outs[0].items():
            assert torch.equal(v, outs[1][k]), (c, m, k)
    from torch_m3gnet.nn.modules import _Topology
    assert _Topology.of(cases[-1]).status() == 0   # no in-launch wait ran into its bound


def test_dp1_rows_in_list_order_are_bit_identical():
    """Option dp1_by_dst: the exact-fp32 reverse edge kernels store each edge's dL/dp1 row at the edge's position in the by-neighbour
    list (Topo::in_pos), so the node reverse streams an atom's rows instead of gathering them.  Same rows, same summation order:
    forces equal bit for bit, through the split-tile and the persistent kernels, on fixtures and on a 2,048-atom cell."""
    from helpers import fcc_cu_graph
    from torch_m3gnet.data import MaterialGraphKey as K

    cases = [(engine_graph(load_oracle_case(c, m)[3]), (c, m)) for c, m in (("cu32fit", "doc"), ("mixfit", "doc"), ("tri", "doc"))]
    cases.append((fcc_cu_graph(8, 8, 8).to("cuda"), ("cu32fit", "doc")))
    for g0, (c, m) in cases:
        for small_tiles in (1 << 20, 0):
            outs = []
            for by_dst in (1, 0):
                model, _ = build_engine_model(c, m)
                model.engine.set_option("small_tiles", small_tiles)
                if small_tiles == 0:
                    model.engine.set_option("split_tail", 0)   # every tile through the whole-tile body of k_edge_rev_f32: its in_pos addressing
                model.engine.set_option("dp1_by_dst", by_dst)
                g = model(g0.clone() if hasattr(g0, "clone") else g0)
                outs.append({k: g[k].clone() for k in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)})
            for k, v in outs[0].items():
                assert torch.equal(v, outs[1][k]), (c, m, small_tiles, k)


# ------------------------------------------------------------------ the size regimes of the kernel selection (round 6)
# Between the fixtures (<= 128 atoms) and BASELINE configs 2 / 3 the step changes kernels by size (plan options small_tiles /
# small_tiles_fwd, split_node_tiles; kFusedSumsMaxAtoms, kNodeTbFusedMaxAtoms in csrc/m3g_internal.h).  These cells sit in every
# regime between the switches.  Reference behaviour held: nn/gradient.py:25-64, tests/test_model.py:59-78.
REGIME_CELLS = [(5, 5, 5),    # 500 atoms, 1,313 tiles: both edge kernels split, >= 3 tiles per workgroup pass
                (6, 6, 6),    # 864 atoms, 2,268 tiles: split forward + persistent reverse by default
                (7, 7, 7)]    # 1,372 atoms, 3,602 tiles: both persistent, fused per-structure sums off


def _fitted_model():
    """The default architecture with the LJ-fitted weights (|F| ~ 1 eV/A: activations away from their linear range), `doc` factors."""
    model, _ = build_engine_model("cu32fit", "doc")
    return model


def _regime_outputs(model, g0, **options):
    from torch_m3gnet.data import MaterialGraphKey as K

    for name, value in options.items():
        model.engine.set_option(name, value)
    g = model(g0.clone())
    torch.cuda.synchronize()
    return {k: g[k].clone() for k in (K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR, K.MID_EDGE_FEATURES,
                                      K.FORCES, K.STRESSES)}


@pytest.mark.parametrize("cells", REGIME_CELLS)
def test_small_path_equals_large_path_in_every_size_regime(cells):
    """500 / 864 / 1,372-atom Cu cells with the split-tile kernels forced on (small_tiles = 2^20), forced off (0) and on the
    DEFAULT selection: forward outputs bit-identical across all three, forces and stresses within 1e-5 of their largest component."""
    from helpers import fcc_cu_graph
    from torch_m3gnet.data import MaterialGraphKey as K

    g0 = fcc_cu_graph(*cells).to("cuda")
    forced = _regime_outputs(_fitted_model(), g0, small_tiles=1 << 20)
    large = _regime_outputs(_fitted_model(), g0, small_tiles=0)
    default = _regime_outputs(_fitted_model(), g0)
    for name, other in (("split", forced), ("default", default)):
        for k in (K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR, K.MID_EDGE_FEATURES):
            assert torch.equal(other[k], large[k]), (cells, name, k)
        assert rel_err(other[K.FORCES], large[K.FORCES]) < 1e-5, (cells, name)
        assert rel_err(other[K.STRESSES], large[K.STRESSES]) < 1e-5, (cells, name)
    # the mixed regime itself, whatever the defaults are: split forward + persistent reverse, and the other way round
    mixed = _regime_outputs(_fitted_model(), g0, small_tiles=0, small_tiles_fwd=1 << 20)
    assert torch.equal(mixed[K.EDGE_ATTR], large[K.EDGE_ATTR]) and torch.equal(mixed[K.TOTAL_ENERGY], large[K.TOTAL_ENERGY])
    assert torch.equal(mixed[K.FORCES], large[K.FORCES])   # same reverse kernels on bit-identical saved activations
    mixed2 = _regime_outputs(_fitted_model(), g0, small_tiles=1 << 20, small_tiles_fwd=0)
    assert torch.equal(mixed2[K.EDGE_ATTR], large[K.EDGE_ATTR])
    assert torch.equal(mixed2[K.FORCES], forced[K.FORCES])


def _vs_fp64_oracle(model, out, e_tol=1e-5, f_tol=1e-4, m_tol=1e-4):
    """Engine outputs against the fp64 evaluation of the oracle (exact derivative) on the same inputs and captured constants."""
    import dataclasses

    from oracle import m3gnet_oracle as orc
    from test_gpu_properties import _oracle_inputs
    from torch_m3gnet.data import MaterialGraphKey as K

    torch.set_num_threads(8)
    p, cfg, c, og = _oracle_inputs(model, out)
    p64 = {k: v.double() for k, v in p.items()}
    c64 = dataclasses.replace(c, **{f.name: getattr(c, f.name).double() for f in dataclasses.fields(c)})
    o = orc.energy_forces(p64, cfg, c64, og, legendre_backward="exact")
    e_err = float(((out[K.TOTAL_ENERGY].double().cpu() - o["total_energy"]).abs() / o["total_energy"].abs()).max())
    f_err = rel_err(out[K.FORCES], o["forces"])
    m_err = max(rel_err(out[K.MID_EDGE_FEATURES][b], o[f"mid_edge_features_{b}"]) for b in range(cfg.num_blocks))
    assert e_err < e_tol and f_err < f_tol and m_err < m_tol, (e_err, f_err, m_err)
    return e_err, f_err, m_err


def test_mid_size_cell_on_the_default_selection_vs_oracle():
    """The 864-atom Cu cell (the size every mid-size figure is quoted on) with the LJ-fitted weights in `doc` mode on the DEFAULT
    kernel selection against the CPU oracle: E 1e-5, F 1e-4 of max|F|, mid_edge_features 1e-4 in every block."""
    from helpers import fcc_cu_graph

    model = _fitted_model()
    out = model(fcc_cu_graph(6, 6, 6).to("cuda"))
    margins = _vs_fp64_oracle(model, out)
    import os
    if os.path.isdir("gpurun_out"):
        with open("gpurun_out/mid_size_margins.txt", "a") as fh:
            fh.write("864-atom cell, default selection vs oracle: E %.2e  F %.2e  mid_edge_features %.2e\n" % margins)


def test_many_small_structures_beyond_the_fused_launches_limit_vs_oracle():
    """One batch of 12 x 64-atom random-species cells (more structures than the fused launches walk, kForceTailMaxStructs = 8:
    the stand-alone sum kernels run) against the oracle, and batched == per-structure energies (reference tests/test_model.py:59-78)."""
    from helpers import random_cell_graph
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.material_graph import Batch
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(3)
    model = build_model(cutoff=5.0, threebody_cutoff=4.0, l_max=3, n_max=3, num_types=95, embedding_dim=64, num_blocks=3)
    for m in model.model:
        if type(m).__name__ == "ThreeBodyInteration":
            m.nsb.factors = m.nsb.documented_factors()
    cells = [random_cell_graph(64, 9.1, s) for s in range(12)]
    out = model(Batch.from_data_list(cells).to("cuda"))
    assert out[K.TOTAL_ENERGY].numel() == 12
    _vs_fp64_oracle(model, out)
    e_all = out[K.TOTAL_ENERGY].clone()
    for s in (0, 7, 11):
        one = model(Batch.from_data_list([cells[s]]).to("cuda"))
        torch.testing.assert_close(one[K.TOTAL_ENERGY], e_all[s:s + 1], rtol=1e-6, atol=1e-6)


def test_in_launch_wait_that_runs_out_poisons_the_forces():
    """k_node_tb_reverse (cells of at most 128 atoms): the node role waits inside the launch for the three-body role's rows.  The
    launcher takes that form only when the runtime says every workgroup of the launch is resident at once; the wait is bounded all
    the same, and when it runs out (forced here: option debug_node_tb_polls < 0 makes the node role wait for an increment that never
    comes) the call must not hand out numbers computed from rows that were never published: forces NaN, sticky M3G_TOPO_ERR_SYNC."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.modules import _Topology

    model, _ = build_engine_model("cu32fit", "doc")
    _, _, _, graph, _ = load_oracle_case("cu32fit", "doc")
    good = model(engine_graph(graph))
    f_good = good[K.FORCES].clone()
    assert torch.isfinite(f_good).all() and _Topology.of(good).status() == 0
    model.engine.set_option("debug_node_tb_polls", -64)
    bad = model(engine_graph(graph))
    assert torch.isnan(bad[K.FORCES]).any()
    assert torch.equal(bad[K.TOTAL_ENERGY], good[K.TOTAL_ENERGY])   # (the forward pass is untouched)
    assert _Topology.of(bad).status() & 2
    model.engine.set_option("debug_node_tb_polls", 0)
    again = model(engine_graph(graph))
    assert torch.equal(again[K.FORCES], f_good) and _Topology.of(again).status() == 0
    # a generous bound on the real wait changes nothing
    model.engine.set_option("debug_node_tb_polls", 1 << 20)
    assert torch.equal(model(engine_graph(graph))[K.FORCES], f_good)


@pytest.mark.parametrize("cells,mode", [((6, 6, 6), 1), ((8, 8, 8), 1), ((5, 5, 5), 2), ((9, 9, 9), 2)])
def test_split_tail_of_the_persistent_reverse_kernel(cells, mode):
    """Option split_tail (default 1): the single tile a workgroup of the persistent reverse kernel cannot share out over its four SIMDs
    goes through the four-way split once its whole tiles are done (rev_split_run inside k_edge_rev_f32).  864 atoms: 9 tiles per
    workgroup -> 8 whole + 1 split; 2,048 atoms: 21 -> 20 + 1.  Mode 2 (opt-in) also takes two left-over tiles, one per group of four
    waves: 500 atoms (persistent kernels forced) 6 -> 4 + 2, 2,916 atoms 30 -> 28 + 2.  Forward outputs do not depend on the option;
    forces and stresses agree with the all-whole-tiles kernel to 1e-5 of their largest component (the split associates dL/dh and dL/dm
    per wave); every setting deterministic."""
    from helpers import fcc_cu_graph
    from torch_m3gnet.data import MaterialGraphKey as K

    g0 = fcc_cu_graph(*cells).to("cuda")
    with_tail = _regime_outputs(_fitted_model(), g0, small_tiles=0, split_tail=mode)
    whole = _regime_outputs(_fitted_model(), g0, small_tiles=0, split_tail=0)
    for k in (K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES, K.EDGE_ATTR, K.MID_EDGE_FEATURES):
        assert torch.equal(with_tail[k], whole[k]), (cells, k)
    f_err, s_err = rel_err(with_tail[K.FORCES], whole[K.FORCES]), rel_err(with_tail[K.STRESSES], whole[K.STRESSES])
    assert 0.0 < f_err < 1e-5 and s_err < 1e-5, (cells, f_err, s_err)   # (> 0: the tail really ran)
    again = _regime_outputs(_fitted_model(), g0, small_tiles=0, split_tail=mode)
    assert torch.equal(again[K.FORCES], with_tail[K.FORCES]) and torch.equal(again[K.STRESSES], with_tail[K.STRESSES])
    import os
    if os.path.isdir("gpurun_out"):
        with open("gpurun_out/small_vs_large_margins.txt", "a") as fh:
            fh.write(f"split tail, {4 * cells[0] ** 3} atoms: forward bit-identical; F {f_err:.2e} of max|F|, stress {s_err:.2e}\n")


def test_split_tail_with_the_references_legendre_backward_on_a_fixture():
    """mixfit / doc (one tile per workgroup: under split_tail = 1 every tile goes through rev_split_run, under 0 through the whole-tile
    body) with legendre_backward = 1: both settings reproduce the reference's own forces at 1e-5 of max|F|, the gate of
    test_reference_legendre_backward_reproduces_the_references_forces (tests/test_gpu_parity.py)."""
    from helpers import persistent_tile_counts, record_line
    from torch_m3gnet.data import MaterialGraphKey as K

    _, _, _, graph, expect = load_oracle_case("mixfit", "doc")
    assert max(persistent_tile_counts(graph["edge_index"].shape[1])) == 1
    forces = {}
    for split_tail in (0, 1):
        model, _ = build_engine_model("mixfit", "doc")
        for name, value in dict(small_tiles=0, split_tail=split_tail, legendre_backward=1).items():
            model.engine.set_option(name, value)
        forces[split_tail] = model(engine_graph(graph))[K.FORCES].clone()
        err = rel_err(forces[split_tail], expect["out_forces"])
        record_line("small_vs_large_margins.txt", f"mixfit_doc legendre_backward=1, persistent reverse kernel, split_tail {split_tail}: F vs the reference {err:.2e}")
        assert err < 1e-5, (split_tail, err)
    assert 0.0 < rel_err(forces[1], forces[0]) < 1e-5   # two bodies, not one


@pytest.mark.parametrize("forces", [True, False])
def test_split_node_and_readout_kernels_are_bit_identical(forces):
    """Option split_node_tiles alone: 128 (default: split node tables, k_geometry_node_pre, split readout) against 0
    (k_node_pre_mfma<fp32>, k_readout_mfma<fp32>), every other option at its default -- the split forms run the same k-ordered
    chains, so energies, per-atom energies, node features, forces and stresses are equal bit for bit.  One part-filled 16-atom
    tile, 108 atoms (six full tiles and a part-filled seventh) and a batch of three structures (the launch's last workgroup walks
    more than one); forces=False is the GRAD = false instantiation of the split readout."""
    from helpers import fcc_cu_graph, random_cell_graph
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.material_graph import Batch

    graphs = [Batch.from_data_list([random_cell_graph(12, 6.0, 0)]).to("cuda"), fcc_cu_graph(3, 3, 3).to("cuda"),
              Batch.from_data_list([random_cell_graph(12, 6.0, s) for s in range(3)]).to("cuda")]
    keys = [K.TOTAL_ENERGY, K.SCALED_ATOMIC_ENERGIES, K.NODE_FEATURES] + ([K.FORCES, K.STRESSES] if forces else [])
    for i, g0 in enumerate(graphs):
        outs = []
        for tiles in (128, 0):
            model, _ = build_engine_model("cu32", "doc")
            model.engine.set_option("split_node_tiles", tiles)
            g = model(g0.clone(), forces=forces)
            torch.cuda.synchronize()
            outs.append({k: g[k].clone() for k in keys})
        for k in keys:
            assert torch.equal(outs[0][k], outs[1][k]), (i, k)
