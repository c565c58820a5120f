"""CPU: the yardstick of tests/test_gpu_standalone_modules.py.  The module-by-module restatements of tests/standalone_cases.py reproduce
the reference's golden stage outputs; the numpy restatement (the second fp32 order, which also carries the scales) equals the oracle's
in fp64; the second order stays within MARGIN / 2 units; and the host check that ThreeBodyInteration.forward and
AtomWiseReadout.forward run before their kernels refuses every out-of-range index tensor."""
import numpy as np
import pytest
import torch

import standalone_cases as sc
from helpers import load_oracle_case, rel_err


def _module_params(params, idx):
    prefix = f"model.{idx}."
    return {k[len(prefix):]: v.numpy() for k, v in params.items() if k.startswith(prefix)}


@pytest.mark.parametrize("case,mode", [("cu32", "ref"), ("tri", "ref"), ("mix", "doc")])
def test_module_by_module_restatement_reproduces_the_golden_stages(case, mode):
    torch.set_num_threads(1)
    params, cfg, consts, graph, expect = load_oracle_case(case, mode)
    g = {k: v.numpy() for k, v in graph.items()}
    f32, tol = torch.float32, 1e-6
    dist, ang = sc.ref_distance_angle(g, cfg.length_scale, f32)
    assert rel_err(torch.tensor(dist), expect["out_edge_distances"]) < tol
    ew = sc.ref_edge_weights(dist, cfg, consts, f32)
    assert rel_err(torch.tensor(ew), expect["out_edge_weights"]) < tol
    x = params["model.3.linear.weight"].numpy().T[g["atom_types"]]                      # AtomFeaturizer: a row gather
    assert np.array_equal(x, expect["mid_x0"].numpy())
    e = sc.ref_linear(ew, params["model.5.linear.weight"].numpy(), None, 1, f32)         # EdgeAdjustor
    assert rel_err(torch.tensor(e), expect["mid_edge_attr0"]) < tol
    for b in range(cfg.num_blocks):
        tb = dict(graph=g, cfg=cfg, consts=consts, params=_module_params(params, 6 + 2 * b), dist=dist, angles=ang, x=x, e=e)
        mid, e = sc.ref_three_body(tb, f32)
        assert rel_err(torch.tensor(mid), expect[f"mid_mid_edge_features_{b}"]) < tol, b
        x, e = sc.ref_conv(dict(graph=g, params=_module_params(params, 7 + 2 * b), x=x, e=e, h=ew), f32)
        assert rel_err(torch.tensor(x), expect[f"mid_x_{b}"]) < tol, b
    assert rel_err(torch.tensor(x), expect["out_x"]) < tol and rel_err(torch.tensor(e), expect["out_edge_attr"]) < tol
    ro = dict(params=_module_params(params, 6 + 2 * cfg.num_blocks), x=x, elemental=consts.elemental_energies.numpy()[g["atom_types"]],
              batch=g["batch"], S=g["lattice"].shape[0], energy_scale=cfg.energy_scale)
    ea, st, tot = sc.ref_readout(ro, f32)
    for mine, theirs in ((ea, "out_scaled_atomic_energies"), (st, "out_scaled_total_energy"), (tot, "out_total_energy")):
        assert rel_err(torch.tensor(mine), expect[theirs]) < tol, theirs


def test_numpy_restatement_equals_the_oracles_in_fp64():
    """The scales are those of the values they stand beside: the numpy restatement, which carries them, is the oracle's function."""
    f64, worst = torch.float64, {}
    for shape in sc.THREE_BODY_SHAPES:
        case = sc.three_body_case(*shape)
        for name, a, b in zip(("mid_edge_features", "edge_attr_tb"), sc.np_three_body(case, np.float64), sc.ref_three_body(case, f64)):
            worst[name] = max(worst.get(name, 0), sc.scaled(a.v - b, a.s))
    for shape in sc.CONV_SHAPES:
        case = sc.conv_case(*shape)
        for name, a, b in zip(("x_conv", "edge_attr_conv"), sc.np_conv(case, np.float64), sc.ref_conv(case, f64)):
            worst[name] = max(worst.get(name, 0), sc.scaled(a.v - b, a.s))
    for shape in sc.READOUT_SHAPES:
        case = sc.readout_case(*shape)
        for name, a, b in zip(sc.READOUT_OUTPUTS, sc.np_readout(case, np.float64), sc.ref_readout(case, f64)):
            worst[name] = max(worst.get(name, 0), sc.scaled(a.v - b, a.s))
    for degree in (1, 4, 5, 10):
        cfg, c = sc.radial_constants(degree, sc.EDGE_CUTOFF)
        a = sc.np_edge_weights(sc.edge_distances(257), cfg, c, np.float64)
        worst["edge_weights"] = max(worst.get("edge_weights", 0), sc.scaled(a.v - sc.ref_edge_weights(sc.edge_distances(257), cfg, c, f64), a.s))
    for l, n in sc.BESSEL_CORNERS:
        cfg, c = sc.basis_constants(l, n, sc.BESSEL_CUTOFF)
        a = sc.np_chi(sc.bessel_radii(257), cfg, c, np.float64)
        worst["bessel"] = max(worst.get("bessel", 0), sc.scaled(a.v - sc.ref_bessel(sc.bessel_radii(257), cfg, c, f64), a.s))
    for g in sc.geometry_graphs().values():
        for name, a, b in zip(("edge_distances", "triplet_angles"), sc.np_distance_angle(g, 1.7, np.float64), sc.ref_distance_angle(g, 1.7, f64)):
            worst[name] = max(worst.get(name, 0), sc.scaled(a.v - b, a.s))
    print(worst)
    # fp64 rounding (1e-16) through the same terms: three orders of magnitude of room, five below the fp32 units
    assert all(v < 1e-12 for v in worst.values()), worst


def test_margin_covers_a_second_fp32_order():
    """MARGIN / 2 units hold the numpy restatement in fp32 (K summed backwards, numpy's libm, other associations)."""
    units = sc.all_units()
    assert set(units) == set(sc.MARGIN)
    for name, (unit, second) in units.items():
        print(f"{name:24s} unit {unit:.3e}  second fp32 order {second / unit:.2f} units  MARGIN {sc.MARGIN[name]}")
        assert 0 < unit < 1e-5, (name, unit)                      # an fp32 rounding, not a mistake of the restatement
        assert second <= sc.MARGIN[name] / 2 * unit, (name, second / unit)


def test_the_inputs_are_read_only_and_cover_the_edges():
    x, w, b = sc.linear_case(65, 17, 65)
    with pytest.raises(ValueError):
        x[0, 0] = 1.0
    d = sc.edge_distances(257)
    rc = np.float32(sc.EDGE_CUTOFF)
    assert d[0] == 0 and d[1] == np.float32(1e-4) and d[2] == rc and d[3] < rc < d[4] and d[5] > rc and d.shape == (257,)
    hub = sc.three_body_case(3, 3, 64)["graph"]
    assert int((hub["triplet_edge_index"][0] == 0).sum()) == 300                        # one edge, 300 triplets
    conv = sc.conv_case(64, 10)["graph"]
    assert int((conv["edge_index"][0] == 0).sum()) == 70 and np.all(np.diff(conv["edge_index"][0]) >= 0)
    ro = sc.readout_case(64, 65, 4, 1.0)
    assert np.any(np.diff(ro["batch"]) < 0) and 3 not in ro["batch"] and ro["S"] == 4    # unsorted; the last structure holds no atom
    g = sc.geometry_graphs()
    assert g["E0"]["edge_index"].shape[1] == 0 and g["T0"]["edge_index"].shape[1] > 0 and g["T0"]["triplet_edge_index"].shape[1] == 0
    assert np.linalg.det(g["tri"]["lattice"][0].astype(np.float64)) < 0


def test_edge_featurizer_accepts_every_degree_build_model_accepts():
    """m3g_edge_featurizer decides on n_max before it touches the device: 1..10 pass that decision (E = 0: nothing to launch; without a
    GPU the call then ends in the runtime's own error, which is not the refusal), 0 and 11 are refused as unsupported."""
    from torch_m3gnet import _lib

    lib, a = _lib.load_library(), np.ones(11, np.float32)
    for n_max in range(0, 12):
        status = lib.m3g_edge_featurizer(n_max, 5.0, a.ctypes.data, a.ctypes.data, a.ctypes.data, 0, None, None, None)
        if 1 <= n_max <= 10:
            assert status != _lib.M3G_ERR_UNSUPPORTED, n_max
        else:
            assert status == _lib.M3G_ERR_UNSUPPORTED and b"1..10" in lib.m3g_last_error(), n_max


def test_distance_angle_accepts_the_empty_outputs_of_a_graph_without_edges():
    """E = 0: the distances and angles are empty tensors, whose pointers are null -- not a bad argument (it was refused as one, so
    DistanceAndAngle.forward raised on a cell whose atoms are out of each other's reach).  With edges a null output still is."""
    from torch_m3gnet import _lib

    lib, topo, pos = _lib.load_library(), np.zeros(1 << 16, np.uint8), np.zeros(9, np.float32)
    args = (pos.ctypes.data, pos.ctypes.data, None, topo.ctypes.data, None, None, None, None, None)
    assert lib.m3g_distance_angle(1.0, 3, 0, 0, 1, *args) != _lib.M3G_ERR_VALUE
    assert lib.m3g_distance_angle(1.0, 3, 2, 0, 1, *args) == _lib.M3G_ERR_VALUE and b"null argument" in lib.m3g_last_error()


# ------------------------------------------------------------------------------------------------------ the index refusals
def _lists():
    g = sc.index_graph(6, 4, 3)
    return {k: torch.tensor(np.array(g[k])) for k in ("edge_index", "triplet_edge_index", "batch")}, 6, g["edge_index"].shape[1], 3


def test_host_check_accepts_a_valid_graph_and_empty_lists():
    from torch_m3gnet.nn.modules import check_index_ranges

    g, N, E, S = _lists()
    check_index_ranges(N, E, S, **g)
    check_index_ranges(N, 0, S, edge_index=torch.zeros(2, 0, dtype=torch.long), triplet_edge_index=torch.zeros(2, 0, dtype=torch.long), batch=g["batch"])
    check_index_ranges(0, 0, 2, batch=torch.zeros(0, dtype=torch.long))
    check_index_ranges(N, E, S, edge_index=g["edge_index"].int())


@pytest.mark.parametrize("key,where,value", [
    ("edge_index", (1, 2), 6), ("edge_index", (0, 0), -1), ("edge_index", (1, 0), 2**40),
    ("triplet_edge_index", (0, 1), "E"), ("triplet_edge_index", (1, 0), -1), ("triplet_edge_index", (1, 3), 2**31),
    ("batch", (4,), 3), ("batch", (0,), -1)])
def test_host_check_refuses_an_index_out_of_range(key, where, value):
    from torch_m3gnet.nn.modules import check_index_ranges

    g, N, E, S = _lists()
    g[key][where] = E if value == "E" else value
    with pytest.raises(ValueError, match="out of range"):
        check_index_ranges(N, E, S, **g)


def test_host_check_refuses_lists_of_the_wrong_shape_or_type():
    from torch_m3gnet.nn.modules import check_index_ranges

    g, N, E, S = _lists()
    with pytest.raises(ValueError, match="shape"):
        check_index_ranges(N, E + 1, S, edge_index=g["edge_index"])                      # fewer edges than the edge arrays have rows
    with pytest.raises(ValueError, match="shape"):
        check_index_ranges(N + 1, E, S, batch=g["batch"])
    with pytest.raises(ValueError, match="shape"):
        check_index_ranges(N, E, S, triplet_edge_index=g["triplet_edge_index"].reshape(-1))
    with pytest.raises(ValueError, match="integer"):
        check_index_ranges(N, E, S, batch=g["batch"].float())
    with pytest.raises(ValueError, match="out of range"):
        check_index_ranges(N, E, 0, batch=g["batch"])                                    # no structure at all
