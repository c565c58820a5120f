"""GPU: stand-alone `forward` of the block modules (EdgeAdjustor, GatedMLP, NormalizedSphericalBessel, ThreeBodyInteration,
M3GNetConv, AtomWiseReadout) -- the reference calls the bare Sequential in tests/test_model.py:14-38.  Each module runs its own
C-ABI stage kernel; checked against the fused engine call, against plain torch fp32 on the CPU (single ops), and through the
reference's triplet-permutation property.  Second half: every module on its own with known inputs (tests/standalone_cases.py) against
an fp64 restatement, element by element in units of the restatement's own fp32 rounding; the scratch-taking entry points on guarded
buffers of exactly the size include/m3gnet_hip.h documents; inputs left untouched; out-of-range index tensors refused on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import standalone_cases as sc
from guarded import Arena
from helpers import record_line, rel_err
from test_gpu_properties import _al_na, _default_model, _oracle_inputs, _small_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _K():
    from torch_m3gnet.data import MaterialGraphKey as K

    return K


@pytest.mark.parametrize("which", ["small", "default", "wide", "ls17", "n6l5"])
def test_bare_sequential_matches_the_fused_call_and_the_oracle(which):
    from oracle import m3gnet_oracle as orc
    from helpers import random_cell_graph
    from torch_m3gnet.data.material_graph import Batch
    from torch_m3gnet.model.build import build_model

    K = _K()
    if which == "small":
        model, cells = _small_model(), _al_na(True)
    elif which == "default":
        model = _default_model(energy_scale=2.0, elemental_energies=torch.linspace(-1, 1, 95))
        cells = [random_cell_graph(18, 6.2, s) for s in (4, 5)]
    elif which == "ls17":   # a length scale: every cutoff and every distance of the bare Sequential is a scaled one
        model = _default_model(energy_scale=2.0, length_scale=1.7, elemental_energies=torch.linspace(-1, 1, 95))
        cells = [random_cell_graph(18, 6.2, s) for s in (4, 5)]
    else:   # sizes only the any-size kernels handle; "n6l5": a radial degree beyond the MFMA path's four
        torch.manual_seed(3)
        model = build_model(4.5, 4.0, 5, 4, 40, 96, 2) if which == "wide" else build_model(4.5, 4.0, 5, 6, 40, 24, 2)
        for m in model.model:
            if type(m).__name__ == "ThreeBodyInteration":
                m.nsb.factors = m.nsb.documented_factors()
        cells = [random_cell_graph(15, 6.0, 9, cutoff=4.5, tb_cutoff=4.0, zmax=39)]
    model = model.to(DEV)
    g = Batch.from_data_list(cells).to(DEV)
    fused = model(g.clone())
    bare = model.model(g.clone())             # module by module, as reference tests/test_model.py:14-18 does
    for key in (K.NODE_FEATURES, K.EDGE_ATTR, K.SCALED_ATOMIC_ENERGIES):
        assert torch.isfinite(bare[key]).all(), key
    assert rel_err(bare[K.NODE_FEATURES], fused[K.NODE_FEATURES]) < 1e-5
    assert rel_err(bare[K.EDGE_ATTR], fused[K.EDGE_ATTR]) < 1e-5
    assert rel_err(bare[K.EDGE_DISTANCES], fused[K.EDGE_DISTANCES]) < 1e-6
    assert rel_err(bare[K.SCALED_ATOMIC_ENERGIES], fused[K.SCALED_ATOMIC_ENERGIES]) < 1e-5
    assert float(((bare[K.TOTAL_ENERGY] - fused[K.TOTAL_ENERGY]).abs() / fused[K.TOTAL_ENERGY].abs()).max()) < 1e-5
    p, cfg, c, og = _oracle_inputs(model, fused)
    o = orc.energy_forces(p, cfg, c, og, want_forces=False)
    assert float(((bare[K.TOTAL_ENERGY].cpu() - o["total_energy"]).abs() / o["total_energy"].abs()).max()) < 1e-5
    n_blocks = (len(model.model) - 7) // 2
    if which != "small":   # (the Al/Na neighbours sit exactly on the three-body cutoff: their aggregate is ~1e-18, pure rounding)
        assert rel_err(bare[K.MID_EDGE_FEATURES], o[f"mid_edge_features_{n_blocks - 1}"]) < 1e-4


def test_edge_features_invariant_under_triplet_permutation():
    """reference tests/test_model.py:21-38, on the stand-alone modules."""
    from torch_m3gnet.data.material_graph import Batch

    K = _K()
    model = _small_model().to(DEV)
    g = Batch.from_data_list(_al_na(True)).to(DEV)
    a = model.model(g.clone())[K.EDGE_ATTR]
    g2 = g.clone()
    perm = torch.randperm(g2[K.TRIPLET_EDGE_INDEX].size(1), generator=torch.Generator().manual_seed(0)).to(DEV)
    g2[K.TRIPLET_EDGE_INDEX] = g2[K.TRIPLET_EDGE_INDEX][:, perm].contiguous()
    b = model.model(g2)[K.EDGE_ATTR]
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("in_features,dims,is_output,use_bias", [(9, [64], False, False), (192, [64, 64], False, True), (17, [33, 5, 1], True, True)])
def test_gated_mlp_forward_against_plain_torch(in_features, dims, is_output, use_bias):
    """GatedMLP.forward on its own (reference nn/core.py:61-62) against the same layers evaluated by plain torch fp32 on the CPU."""
    from torch_m3gnet.nn.core import GatedMLP

    torch.manual_seed(1)
    mlp = GatedMLP(in_features, dims, is_output=is_output, use_bias=use_bias)
    x = torch.randn(37, in_features)
    ref = torch.nn.Sequential(*mlp.dense)(x) * torch.nn.Sequential(*mlp.gate)(x)
    out = mlp.to(DEV)(x.to(DEV))
    assert out.shape == ref.shape
    torch.testing.assert_close(out.cpu(), ref.detach(), rtol=2e-5, atol=2e-6)


def test_normalized_spherical_bessel_forward():
    from torch_m3gnet.nn.interaction import NormalizedSphericalBessel
    from torch_m3gnet.nn.modules import spherical_bessel

    nsb = NormalizedSphericalBessel(cutoff=4.2, l_max=4, n_max=5)
    nsb.factors = nsb.documented_factors()
    rs = torch.linspace(0.0, 4.2, 57)
    out = nsb(rs.to(DEV)).cpu()
    assert out.shape == (4, 5, 57)
    z = nsb.spherical_bessel_zeros[:4, :5].double()
    well = rs >= 0.6
    for l in range(4):
        # The reference's fp32 upward recurrence (nn/interaction.py:293-318) is ill-conditioned at small arguments for l >= 2:
        # on the CPU it is itself 1e-4 away from the fp64 value there (l = 3), so the exact comparison covers r >= 0.6, where
        # it is good to 4e-7, and the small-argument region is held to that noise level.
        ref = spherical_bessel(z[l][:, None] * rs.double()[None, :] / 4.2, l) / nsb.factors[l].double()[:, None]
        err = (out[l].double() - ref).abs()
        assert float(err[:, well].max()) < 3e-6 * float(ref.abs().max())
        assert float(err.max()) < 1e-3 * float(ref.abs().max())


def test_normalized_spherical_bessel_small_arguments_against_the_reference():
    """r in [0, 0.6] A, where the reference's fp32 upward recurrence (nn/interaction.py:293-318) is ill-conditioned: the
    stand-alone kernel against the reference's OWN fp32 output (fixture nsb_small_r.npz, generated by its forward code) and both
    against fp64.  The kernel must be as close to the exact value as the reference is (per l: the reference's own error + 1 % of
    it + 3e-6 of the basis scale -- for l = 3 both are 12 % of the scale away from fp64 and 0.8 % from each other: the recurrence
    amplifies the rounding of sin / cos at x ~ 0.1, whichever libm evaluates them), and where the reference is accurate
    (l <= 1: 3e-6) it must agree with the reference itself."""
    import numpy as np
    from helpers import GOLDEN
    from torch_m3gnet.nn.interaction import NormalizedSphericalBessel

    z = np.load(GOLDEN / "nsb_small_r.npz")
    nsb = NormalizedSphericalBessel(cutoff=float(z["cutoff"]), l_max=int(z["l_max"]), n_max=int(z["n_max"]))
    nsb.factors = torch.tensor(z["factors"])
    rs = torch.tensor(z["rs"])
    out = nsb(rs.to(DEV)).cpu().double()
    ref32, ref64 = torch.tensor(z["chi_fp32"]).double(), torch.tensor(z["chi_fp64"])
    small = rs <= 0.6
    for l in range(int(z["l_max"])):
        scale = float(ref64[l].abs().max())
        mine = float((out[l] - ref64[l]).abs()[:, small].max())
        theirs = float((ref32[l] - ref64[l]).abs()[:, small].max())
        print(f"l = {l}: kernel vs fp64 {mine / scale:.2e}, reference fp32 vs fp64 {theirs / scale:.2e}, kernel vs reference fp32 "
              f"{float((out[l] - ref32[l]).abs()[:, small].max()) / scale:.2e}  (of the basis scale {scale:.3f})")
        assert mine <= 1.01 * theirs + 3e-6 * scale, (l, mine, theirs)
        if theirs < 3e-6 * scale:
            assert float((out[l] - ref32[l]).abs()[:, small].max()) < 6e-6 * scale
        # beyond the ill-conditioned region the kernel agrees with the reference's fp32 numbers to 3e-6
        assert float((out[l] - ref32[l]).abs()[:, rs >= 0.6].max()) < 3e-6 * scale


# ==================================================================================================================================
# Every stand-alone module on its own, against the fp64 restatements of tests/standalone_cases.py: each output element within
# MARGIN[name] units of its own scale (the rule of that file), and within the bound an earlier test states where there is one.
def _d(a, dtype=None):
    return sc.t(a, dtype).to(DEV)


def _np64(x):
    return x.detach().double().cpu().numpy()


class _Worst:
    """The largest scaled deviation per output of one test, asserted against the rule and recorded with the run."""

    def __init__(self):
        self.worst = {}

    def add(self, name, got, want, scale, where=""):
        got = _np64(got) if torch.is_tensor(got) else got
        assert got.shape == want.shape, (name, where, got.shape, want.shape)
        dev = sc.scaled(got - want, scale)
        self.worst[name] = max(self.worst.get(name, 0.0), dev)
        assert dev <= sc.bound(name), f"{name} {where}: {dev / sc.unit(name):.2f} units (MARGIN {sc.MARGIN[name]}, unit {sc.unit(name):.3e})"

    def record(self, test):
        for name, dev in self.worst.items():
            record_line("standalone_modules.txt", f"{test:44s} {name:24s} unit {sc.unit(name):.3e}  MARGIN {sc.MARGIN[name]}  device {dev / sc.unit(name):5.2f} units")


def _untouched(inputs, snapshot):
    for key, before in snapshot.items():
        assert torch.equal(inputs[key], before), f"the module changed its input '{key}'"


def _twice(module, inputs):
    """module(graph) on two shallow copies of `inputs`; the input tensors must come back bit-identical."""
    snapshot = {k: v.clone() for k, v in inputs.items() if torch.is_tensor(v)}
    a, b = module(dict(inputs)), module(dict(inputs))
    _untouched(inputs, snapshot)
    return a, b


def _guarded(arena, tensor, label):
    """A guarded copy of an input (or in-place) tensor, as float32 / int64 the entry points take."""
    return arena.take_copy(tensor.detach().contiguous(), label)


def _direct_three_body(mod, inputs, arena, fill):
    """m3g_three_body through ctypes with EVERY device buffer between guard bands: the inputs and weights as copies, edge_attr (in place) as
    a copy, mid and the scratch of exactly the header's (N*C + E*C + 2*E*D) floats filled with `fill`."""
    from torch_m3gnet import _cuda, _lib
    from torch_m3gnet.data import MaterialGraphKey as K

    x, ei, tei = inputs[K.NODE_FEATURES], inputs[K.EDGE_INDEX], inputs[K.TRIPLET_EDGE_INDEX]
    N, D, E, T, C_ = x.size(0), x.size(1), ei.size(1), tei.size(1), mod.degree
    z, f = mod.nsb._host_tables()
    b = {k: _guarded(arena, inputs[k], k) for k in (K.EDGE_INDEX, K.TRIPLET_EDGE_INDEX, K.EDGE_DISTANCES, K.TRIPLET_ANGLES, K.NODE_FEATURES, K.EDGE_ATTR)}
    w = [_guarded(arena, t_, f"weight {i}") for i, t_ in enumerate((mod.linear_sigmoid1.weight, mod.linear_sigmoid1.bias,
                                                                    mod.gated_mlp.dense[0].weight, mod.gated_mlp.gate[0].weight))]
    mid = arena.take_like((E, C_), torch.float32, fill, "mid")
    scratch = arena.take(4 * (N * C_ + E * C_ + 2 * E * D), fill, "three-body scratch")
    _lib.check(_lib.load_library().m3g_three_body(
        mod.l_max, mod.n_max, D, float(mod.cutoff), float(mod.threebody_cutoff), z.ctypes.data, f.ctypes.data, N, E, T, b[K.EDGE_INDEX].data_ptr(),
        b[K.TRIPLET_EDGE_INDEX].data_ptr(), b[K.EDGE_DISTANCES].data_ptr(), b[K.TRIPLET_ANGLES].data_ptr(), b[K.NODE_FEATURES].data_ptr(),
        *(t_.data_ptr() for t_ in w), scratch.data_ptr(), b[K.EDGE_ATTR].data_ptr(), mid.data_ptr(), _cuda.stream_ptr()))
    torch.cuda.synchronize()
    for k in (K.EDGE_INDEX, K.TRIPLET_EDGE_INDEX, K.EDGE_DISTANCES, K.TRIPLET_ANGLES, K.NODE_FEATURES):
        assert torch.equal(b[k], inputs[k]), k
    return {K.EDGE_ATTR: b[K.EDGE_ATTR], K.MID_EDGE_FEATURES: mid}


def _direct_conv(mod, inputs, arena, fill):
    """m3g_conv_block through ctypes: weights, edge_weights, x and edge_attr (in place) as guarded copies, scratch of exactly
    m3g_conv_block_scratch_bytes filled with `fill`.  (The topology buffer is the graph's own: tests/test_gpu_guard_bands.py guards it.)"""
    from torch_m3gnet import _cuda, _lib
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.modules import _Topology

    lib, topo = _lib.load_library(), _Topology.of(inputs)
    tensors = []
    for mlp, lin in ((mod.concat_edge_update, mod.edge_linear), (mod.concat_node_update, mod.node_linear)):
        tensors += [mlp.dense[0].weight, mlp.gate[0].weight, mlp.dense[0].bias, mlp.gate[0].bias,
                    mlp.dense[2].weight, mlp.gate[2].weight, mlp.dense[2].bias, mlp.gate[2].bias, lin.weight]
    keep = [_guarded(arena, t_, f"weight {i}") for i, t_ in enumerate(tensors)]
    params = (C.c_void_p * 18)(*[t_.data_ptr() for t_ in keep])
    x, e, h = (_guarded(arena, inputs[k], k) for k in (K.NODE_FEATURES, K.EDGE_ATTR, K.EDGE_WEIGHTS))
    D = x.size(1)
    nbytes = C.c_size_t()
    _lib.check(lib.m3g_conv_block_scratch_bytes(D, topo.E, C.byref(nbytes)))
    assert nbytes.value == 4 * (11 * topo.E * D + 1024)            # what include/m3gnet_hip.h states
    scratch = arena.take(nbytes.value, fill, "conv scratch")
    _lib.check(lib.m3g_conv_block(D, mod.degree, topo.N, topo.E, topo.T, topo.S, topo.buf.data_ptr(), params, h.data_ptr(), x.data_ptr(), e.data_ptr(),
                                  scratch.data_ptr(), nbytes.value, _cuda.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(h, inputs[K.EDGE_WEIGHTS]) and all(torch.equal(a, b.detach()) for a, b in zip(keep, tensors))
    return {K.NODE_FEATURES: x, K.EDGE_ATTR: e}


def _direct_readout(mod, inputs, arena, fill):
    """m3g_readout through ctypes: weights, x, the elemental energies and batch as guarded copies; the three outputs and the scratch of
    exactly the header's (4*N*D + 2*N) floats filled with `fill`."""
    from torch_m3gnet import _cuda, _lib
    from torch_m3gnet.data import MaterialGraphKey as K

    tensors = []
    for seq in (mod.gated.dense, mod.gated.gate):
        for i in (0, 2, 4):
            tensors += [seq[i].weight, seq[i].bias]
    keep = [_guarded(arena, t_, f"weight {i}") for i, t_ in enumerate(tensors)]
    params = (C.c_void_p * 12)(*[t_.data_ptr() for t_ in keep])
    x, elem, batch = (_guarded(arena, inputs[k], k) for k in (K.NODE_FEATURES, K.ELEMENTAL_ENERGIES, K.BATCH))
    N, D = x.shape
    S = inputs[K.LATTICE].size(0)
    ea, st, tot = (arena.take_like((n,), torch.float32, fill, lab) for n, lab in ((N, "scaled_atomic"), (S, "scaled_total"), (S, "total")))
    scratch = arena.take(4 * (4 * N * D + 2 * N), fill, "readout scratch")
    _lib.check(_lib.load_library().m3g_readout(D, N, S, params, float(mod.scale), x.data_ptr(), elem.data_ptr(), batch.data_ptr(), ea.data_ptr(),
                                               st.data_ptr(), tot.data_ptr(), scratch.data_ptr(), _cuda.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(x, inputs[K.NODE_FEATURES]) and torch.equal(batch, inputs[K.BATCH]) and torch.equal(elem, inputs[K.ELEMENTAL_ENERGIES])
    return {K.SCALED_ATOMIC_ENERGIES: ea, K.SCALED_TOTAL_ENERGY: st, K.TOTAL_ENERGY: tot}


def _linear_module(w, b):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None)
    lin.weight.data = _d(w)
    if b is not None:
        lin.bias.data = _d(b)
    return lin.to(DEV)


# ------------------------------------------------------------------------------------------------------------- m3g_linear
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_on_every_tile_edge_against_fp64(act):
    """rows below / on / above one and two 64-row tiles, k around one 16-deep slab and at twelve, columns around one 16-column block and
    around the 64-column tile; with and without bias; through the wrapper and, with bias, through the C entry point on guarded buffers
    under two fills of y (bit-identical, bands intact)."""
    from torch_m3gnet import _cuda, _lib
    from torch_m3gnet.nn.modules import _linear

    lib, w_ = _lib.load_library(), _Worst()
    for k in sc.LINEAR_IN:
        for o in sc.LINEAR_OUT:
            for n in sc.LINEAR_ROWS:
                x, w, b = sc.linear_case(n, k, o)
                for bias in (None, b):
                    y = _linear(_d(x), _linear_module(w, bias), act)
                    assert y.shape == (n, o) and y.dtype == torch.float32
                    w_.add("linear", y, sc.ref_linear(x, w, bias, act, torch.float64), sc.linear_scale(x, w, bias, act), (n, k, o, bias is not None))
                arena = Arena(DEV)
                gx, gw, gb = (arena.take_copy(_d(a), lab) for a, lab in ((x, "x"), (w, "w"), (b, "b")))
                ys = [arena.take_like((n, o), torch.float32, fill, f"y fill {fill:#x}") for fill in (0x00, 0xFF)]
                for gy in ys:
                    _lib.check(lib.m3g_linear(n, k, o, gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), act, gy.data_ptr(), _cuda.stream_ptr()))
                torch.cuda.synchronize()
                arena.check()
                assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], y), (n, k, o)   # (y: the wrapper's, with bias)
    w_.record(f"linear act {act}")


def test_linear_input_layouts():
    """[3, 7, in] keeps its leading shape; a transposed view and an fp64 input give the bits of the contiguous fp32 input, which stays
    untouched."""
    from torch_m3gnet.nn.modules import _linear

    x, w, b = sc.linear_case(130, 17, 65)
    lin, flat = _linear_module(w, b), _d(x)[:21]
    want = _linear(flat, lin, 1)
    cube = flat.reshape(3, 7, 17).clone()
    got = _linear(cube, lin, 1)
    assert got.shape == (3, 7, 65) and torch.equal(got.reshape(21, 65), want) and torch.equal(cube.reshape(21, 17), flat)
    view = flat.t().contiguous().t()
    assert not view.is_contiguous()
    keep = view.clone()
    assert torch.equal(_linear(view, lin, 1), want) and torch.equal(view, keep)
    wide = flat.double()
    out = _linear(wide, lin, 1)
    assert out.dtype == torch.float32 and torch.equal(out, want) and wide.dtype == torch.float64


@pytest.mark.parametrize("shape", sc.GATED_MLP_SHAPES)
def test_gated_mlp_against_fp64(shape):
    from torch_m3gnet.nn.core import GatedMLP

    case = sc.gated_mlp_case(*shape)
    mlp = GatedMLP(shape[0], list(shape[1]), is_output=shape[2], use_bias=shape[3])
    mlp.load_state_dict({k: sc.t(v) for k, v in case["params"].items()})
    x = _d(case["x"])
    keep = x.clone()
    out = mlp.to(DEV)(x)
    assert torch.equal(x, keep) and torch.equal(out, mlp(x))
    w_ = _Worst()
    w_.add("gated_mlp", out, sc.ref_gated_mlp(case["x"], case["params"], len(shape[1]), shape[2], shape[3], torch.float64),
           sc.np_gated_mlp(sc.VS(np.asarray(case["x"], np.float64)), case["params"], "", len(shape[1]), shape[2], shape[3]).s)
    w_.record(f"gated_mlp {shape[0]}->{list(shape[1])}")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_multiply_is_the_fp32_product(n):
    from torch_m3gnet import _cuda, _lib

    rng = np.random.default_rng([sc.SEED, 11, n])
    a, b = (torch.tensor(rng.normal(0, 1, n).astype(np.float32)).to(DEV) for _ in range(2))
    arena = Arena(DEV)
    ys = [arena.take_like((n,), torch.float32, fill) for fill in (0x00, 0xFF)]
    for y in ys:
        _lib.check(_lib.load_library().m3g_multiply(n, a.data_ptr(), b.data_ptr(), y.data_ptr(), _cuda.stream_ptr()))
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(ys[0], a * b) and torch.equal(ys[1], a * b)


# ------------------------------------------------------------------------------------------------ AtomFeaturizer / AtomRef
@pytest.mark.parametrize("num_types", [1, 95])
@pytest.mark.parametrize("dim", [1, 64, 96])
def test_atom_featurizer_and_atom_ref_are_row_gathers(num_types, dim):
    """Rows equal to the columns of linear.weight bit for bit; an out-of-range species gives a NaN row for that atom only."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.atom_ref import AtomRef
    from torch_m3gnet.nn.featurizer import AtomFeaturizer

    rng = np.random.default_rng([sc.SEED, 12, num_types, dim])
    feat = AtomFeaturizer(num_types=num_types, embedding_dim=dim).to(DEV)
    table = torch.tensor(rng.normal(0, 2, num_types).astype(np.float32))
    ref = AtomRef(table).to(DEV)
    w = feat.linear.weight.detach().clone()
    for N in (0, 1, 257):
        types = torch.tensor(rng.integers(0, num_types, N)).to(DEV)
        a, b = _twice(feat, {K.ATOM_TYPES: types})
        assert a[K.NODE_FEATURES].shape == (N, dim) and torch.equal(a[K.NODE_FEATURES], w.t()[types]) and torch.equal(a[K.NODE_FEATURES], b[K.NODE_FEATURES])
        a, b = _twice(ref, {K.ATOM_TYPES: types})
        assert torch.equal(a[K.ELEMENTAL_ENERGIES], table.to(DEV)[types]) and torch.equal(a[K.ELEMENTAL_ENERGIES], b[K.ELEMENTAL_ENERGIES])
    assert torch.equal(feat.linear.weight.detach(), w)
    bad = types.clone()
    bad[5], bad[9] = num_types, -1
    good = torch.ones(257, dtype=torch.bool, device=DEV)
    good[5] = good[9] = False
    x = feat({K.ATOM_TYPES: bad})[K.NODE_FEATURES]
    assert torch.isnan(x[~good]).all() and torch.equal(x[good], w.t()[types][good])
    e = ref({K.ATOM_TYPES: bad})[K.ELEMENTAL_ENERGIES]
    assert torch.isnan(e[~good]).all() and torch.equal(e[good], table.to(DEV)[types][good])


# ---------------------------------------------------------------------------------------------------------- EdgeFeaturizer
@pytest.mark.parametrize("degree", list(range(1, 11)))
def test_edge_featurizer_every_degree_against_fp64(degree):
    """Degrees 1..10 (1..4 on the MFMA path's kernel, 5..10 on the any-size path's radial basis): distances 0, 1e-4, the cutoff, its
    float32 neighbours, beyond it; E = 0, 1, 257."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.featurizer import EdgeFeaturizer

    cfg, c = sc.radial_constants(degree, sc.EDGE_CUTOFF)
    mod, w_ = EdgeFeaturizer(degree=degree, cutoff=sc.EDGE_CUTOFF), _Worst()
    for E in (0, 1, 257):
        d = sc.edge_distances(E)
        a, b = _twice(mod, {K.EDGE_DISTANCES: _d(d)})
        got = a[K.EDGE_WEIGHTS]
        assert got.shape == (E, degree) and torch.equal(got, b[K.EDGE_WEIGHTS])
        want = sc.ref_edge_weights(d, cfg, c, torch.float64)
        w_.add("edge_weights", got, want, sc.np_edge_weights(d, cfg, c, np.float64).s, E)
        if E:
            assert rel_err(got, torch.tensor(want)) < 1e-5
    w_.record(f"edge_featurizer degree {degree}")


# --------------------------------------------------------------------------------------------- NormalizedSphericalBessel
@pytest.mark.parametrize("l_max,n_max", sc.BESSEL_CORNERS)
def test_normalized_spherical_bessel_corners_against_fp64(l_max, n_max):
    from torch_m3gnet.nn.interaction import NormalizedSphericalBessel

    cfg, c = sc.basis_constants(l_max, n_max, sc.BESSEL_CUTOFF)
    nsb = NormalizedSphericalBessel(cutoff=sc.BESSEL_CUTOFF, l_max=l_max, n_max=n_max)
    nsb.factors, nsb.spherical_bessel_zeros = c.factors.clone(), c.zeros.clone()
    w_ = _Worst()
    for n in (0, 1, 257):
        r = sc.bessel_radii(n)
        rs = _d(r)
        keep = rs.clone()
        out = nsb(rs)
        assert out.shape == (l_max, n_max, n) and torch.equal(rs, keep) and torch.equal(out, nsb(rs))
        want = sc.ref_bessel(r, cfg, c, torch.float64)
        w_.add("bessel", out, want, sc.np_chi(r, cfg, c, np.float64).s, n)
        for l in range(min(l_max, 4) if n else 0):   # the orders and radii for which the existing test states 3e-6 of the basis scale
            assert float(np.abs(_np64(out)[l] - want[l]).max()) < 3e-6 * float(np.abs(want[l]).max())
    w_.record(f"bessel l_max {l_max} n_max {n_max}")


# -------------------------------------------------------------------------------------------------------- DistanceAndAngle
def _geometry_inputs(g):
    from torch_m3gnet.data import MaterialGraphKey as K

    return {K.POS: _d(g["pos"]), K.LATTICE: _d(g["lattice"]), K.BATCH: _d(g["batch"]).long(), K.EDGE_INDEX: _d(g["edge_index"]).long(),
            K.EDGE_CELL_SHIFT: _d(g["edge_cell_shift"]), K.TRIPLET_EDGE_INDEX: _d(g["triplet_edge_index"]).long()}


@pytest.mark.parametrize("length_scale", sc.GEOMETRY_SCALES)
@pytest.mark.parametrize("which", ["tri", "pair", "E0", "T0"])
def test_distance_and_angle_against_fp64(which, length_scale):
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.invariant import DistanceAndAngle
    from torch_m3gnet.nn.scale import ScaleLength

    g = sc.geometry_graphs()[which]
    a, b = _twice(torch.nn.Sequential(ScaleLength(length_scale), DistanceAndAngle()), _geometry_inputs(g))
    d64, a64 = sc.ref_distance_angle(g, length_scale, torch.float64)
    sd, sa = sc.np_distance_angle(g, length_scale, np.float64)
    w_ = _Worst()
    w_.add("edge_distances", a[K.EDGE_DISTANCES], d64, sd.s)
    w_.add("triplet_angles", a[K.TRIPLET_ANGLES], a64, sa.s)
    assert torch.equal(a[K.EDGE_DISTANCES], b[K.EDGE_DISTANCES]) and torch.equal(a[K.TRIPLET_ANGLES], b[K.TRIPLET_ANGLES])
    assert a[K.EDGE_DISTANCES].shape == d64.shape and a[K.TRIPLET_ANGLES].shape == a64.shape
    if d64.size:
        assert rel_err(a[K.EDGE_DISTANCES], torch.tensor(d64)) < 1e-6
    w_.record(f"distance_angle {which} length_scale {length_scale}")


def test_collinear_triplets_give_exactly_plus_and_minus_one():
    """One atom in a sheared cell: a neighbour and its mirror image (cos = -1), two images of one neighbour (cos = +1)."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.material_graph import Batch, MaterialGraph
    from torch_m3gnet.nn.invariant import DistanceAndAngle
    from torch_m3gnet.nn.scale import ScaleLength

    lat = np.array([[2.1, 0.3, -0.2], [0.4, 2.3, 0.1], [-0.3, 0.2, 2.2]])
    graph = Batch.from_data_list([MaterialGraph.from_arrays(lat, np.array([[0.37, 0.11, 0.23]]), [29], 4.9, 4.9)])
    g = {k: graph[k].numpy() for k in ("pos", "lattice", "batch", "edge_index", "edge_cell_shift", "triplet_edge_index")}
    _, cos64 = sc.ref_distance_angle(g, 1.7, torch.float64)
    out = torch.nn.Sequential(ScaleLength(1.7), DistanceAndAngle())(_geometry_inputs(g))[K.TRIPLET_ANGLES].cpu().numpy()
    plus, minus = cos64 > 1 - 1e-12, cos64 < -1 + 1e-12
    assert plus.sum() > 0 and minus.sum() > 0
    assert np.all(out[plus] == 1.0) and np.all(out[minus] == -1.0) and np.all(np.abs(out) <= 1.0)


# ----------------------------------------------------------------------------------------------------- ThreeBodyInteration
def _three_body(case):
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.interaction import ThreeBodyInteration

    cfg, g = case["cfg"], case["graph"]
    mod = ThreeBodyInteration(cfg.cutoff, cfg.threebody_cutoff, cfg.l_max, cfg.n_max, case["D"], case["D"])
    mod.load_state_dict({k: sc.t(v) for k, v in case["params"].items()})
    mod.nsb.factors, mod.nsb.spherical_bessel_zeros = case["consts"].factors.clone(), case["consts"].zeros.clone()
    inputs = {K.NODE_FEATURES: _d(case["x"]), K.EDGE_ATTR: _d(case["e"]), K.EDGE_INDEX: _d(g["edge_index"]), K.TRIPLET_EDGE_INDEX: _d(g["triplet_edge_index"]),
              K.EDGE_DISTANCES: _d(case["dist"]), K.TRIPLET_ANGLES: _d(case["angles"])}
    return mod.to(DEV), inputs


@pytest.mark.parametrize("l_max,n_max,D", sc.THREE_BODY_SHAPES)
def test_three_body_against_fp64(l_max, n_max, D):
    """One edge with 300 triplets (contended atomics), the list as built and shuffled, T = 0 and E = 0; `mid` and `edge_attr` against
    fp64, through the wrapper (twice, inputs untouched) and through the C entry point with every buffer guarded and the scratch of exactly
    the header's (N*C + E*C + 2*E*D) floats, under two fills."""
    from torch_m3gnet.data import MaterialGraphKey as K

    w_, C_, between = _Worst(), l_max * n_max, {}
    for kind in ("hub", "T0", "E0"):
        case = sc.three_body_case(l_max, n_max, D, kind)
        mod, inputs = _three_body(case)
        E, T = case["dist"].shape[0], case["angles"].shape[0]
        mid64, e64 = sc.ref_three_body(case, torch.float64)
        smid, se = sc.np_three_body(case, np.float64)
        arena, outs = Arena(DEV), list(_twice(mod, inputs))
        outs += [_direct_three_body(mod, inputs, arena, fill) for fill in (0x00, 0xFF)]
        arena.check()
        if T:   # the caller's list in another order: the same sums
            perm = torch.randperm(T, generator=torch.Generator().manual_seed(1)).to(DEV)
            shuffled = dict(inputs)
            shuffled[K.TRIPLET_EDGE_INDEX], shuffled[K.TRIPLET_ANGLES] = inputs[K.TRIPLET_EDGE_INDEX][:, perm].contiguous(), inputs[K.TRIPLET_ANGLES][perm].contiguous()
            outs.append(mod(shuffled))
        for out in outs:   # (two calls differ by the order of the atomics only: each within the rule, which holds them together)
            assert out[K.MID_EDGE_FEATURES].shape == (E, C_) and out[K.EDGE_ATTR].shape == (E, D)
            w_.add("mid_edge_features", out[K.MID_EDGE_FEATURES], mid64, smid.s, kind)
            w_.add("edge_attr_tb", out[K.EDGE_ATTR], e64, se.s, kind)
        for out in outs[1:]:   # call to call (and list order to list order) the sums move by the order of their atomics: within one unit
            for name, key, s in (("mid_edge_features", K.MID_EDGE_FEATURES, smid.s), ("edge_attr_tb", K.EDGE_ATTR, se.s)):
                apart = sc.scaled(_np64(out[key]) - _np64(outs[0][key]), s)
                between[name] = max(between.get(name, 0.0), apart)
                assert apart <= sc.unit(name), f"{name} {kind}: two calls {apart / sc.unit(name):.2f} units apart"
        if T == 0:   # no triplet: the aggregate is exactly zero and the calls agree bit for bit
            assert not outs[0][K.MID_EDGE_FEATURES].any() and all(torch.equal(o[K.EDGE_ATTR], outs[0][K.EDGE_ATTR]) for o in outs)
        else:   # the max-norm bounds of the bare-Sequential test above, at every shape (figures first, then the assertions)
            worst = [max(rel_err(out[key], torch.tensor(w64)) for out in outs) for key, w64 in ((K.MID_EDGE_FEATURES, mid64), (K.EDGE_ATTR, e64))]
            record_line("standalone_modules.txt", f"{f'three_body l_max {l_max} n_max {n_max} D {D}':44s} max-norm error: mid_edge_features {worst[0]:.2e} "
                                                  f"(bound 1e-4), edge_attr {worst[1]:.2e} (bound 1e-5)")
            assert worst[0] < 1e-4 and worst[1] < 1e-5, worst
    w_.record(f"three_body l_max {l_max} n_max {n_max} D {D}")
    for name, apart in between.items():
        record_line("standalone_modules.txt", f"{f'three_body l_max {l_max} n_max {n_max} D {D}':44s} {name:24s} call to call {apart / sc.unit(name):5.2f} units")


# ------------------------------------------------------------------------------------------------------------- M3GNetConv
def _conv(case):
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.conv import M3GNetConv

    g = case["graph"]
    mod = M3GNetConv(case["R"], case["D"], case["D"])
    mod.load_state_dict({k: sc.t(v) for k, v in case["params"].items()})
    inputs = {K.NODE_FEATURES: _d(case["x"]), K.EDGE_ATTR: _d(case["e"]), K.EDGE_WEIGHTS: _d(case["h"]), K.EDGE_INDEX: _d(g["edge_index"]),
              K.TRIPLET_EDGE_INDEX: _d(g["triplet_edge_index"]), K.BATCH: _d(g["batch"]), K.LATTICE: _d(g["lattice"])}
    return mod.to(DEV), inputs


@pytest.mark.parametrize("D,R", sc.CONV_SHAPES)
def test_conv_block_against_fp64(D, R):
    """65 atoms, one the centre of 70 edges; and the same atoms without edges, where x must come back bit-identical.  Through the wrapper
    (twice, inputs untouched) and through the C entry point with x, edge_attr, edge_weights and the weights guarded and scratch of exactly
    m3g_conv_block_scratch_bytes, under two fills: bit-identical outputs."""
    from torch_m3gnet.data import MaterialGraphKey as K

    w_ = _Worst()
    for kind in ("hub", "E0"):
        case = sc.conv_case(D, R, kind)
        mod, inputs = _conv(case)
        arena, outs = Arena(DEV), list(_twice(mod, inputs))
        outs += [_direct_conv(mod, inputs, arena, fill) for fill in (0x00, 0xFF)]
        arena.check()
        x64, e64 = sc.ref_conv(case, torch.float64)
        sx, se = sc.np_conv(case, np.float64)
        for out in outs:
            assert torch.equal(out[K.NODE_FEATURES], outs[0][K.NODE_FEATURES]) and torch.equal(out[K.EDGE_ATTR], outs[0][K.EDGE_ATTR])
        w_.add("x_conv", outs[0][K.NODE_FEATURES], x64, sx.s, kind)
        w_.add("edge_attr_conv", outs[0][K.EDGE_ATTR], e64, se.s, kind)
        if kind == "E0":
            assert torch.equal(outs[0][K.NODE_FEATURES], inputs[K.NODE_FEATURES]) and outs[0][K.EDGE_ATTR].shape == (0, D)
        else:
            assert rel_err(outs[0][K.NODE_FEATURES], torch.tensor(x64)) < 1e-5 and rel_err(outs[0][K.EDGE_ATTR], torch.tensor(e64)) < 1e-5
    w_.record(f"conv D {D} R {R}")


# -------------------------------------------------------------------------------------------------------- AtomWiseReadout
def _readout(case):
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.readout import AtomWiseReadout

    mod = AtomWiseReadout(case["D"], 3, case["energy_scale"])
    mod.load_state_dict({k: sc.t(v) for k, v in case["params"].items()})
    inputs = {K.NODE_FEATURES: _d(case["x"]).reshape(case["N"], case["D"]), K.BATCH: _d(case["batch"]), K.LATTICE: _d(case["graph"]["lattice"]),
              K.ELEMENTAL_ENERGIES: _d(case["elemental"])}
    return mod.to(DEV), inputs


@pytest.mark.parametrize("D,N,S,energy_scale", sc.READOUT_SHAPES)
def test_readout_against_fp64(D, N, S, energy_scale):
    """An unsorted `batch`, a structure that holds no atom (its sums are exactly 0), no atom at all; per-atom energies and the structures'
    sums against fp64, through the wrapper (twice, inputs untouched) and through the C entry point with every buffer guarded and the scratch
    of exactly the header's (4*N*D + 2*N) floats, under two fills."""
    from torch_m3gnet.data import MaterialGraphKey as K

    case = sc.readout_case(D, N, S, energy_scale)
    mod, inputs = _readout(case)
    arena, outs = Arena(DEV), list(_twice(mod, inputs))
    outs += [_direct_readout(mod, inputs, arena, fill) for fill in (0x00, 0xFF)]
    arena.check()
    want, scales, w_ = sc.ref_readout(case, torch.float64), sc.np_readout(case, np.float64), _Worst()
    keys = (K.SCALED_ATOMIC_ENERGIES, K.SCALED_TOTAL_ENERGY, K.TOTAL_ENERGY)
    for out in outs:   # (the structures' sums are float atomics: two calls may differ by their order, each within the rule)
        assert torch.equal(out[K.SCALED_ATOMIC_ENERGIES], outs[0][K.SCALED_ATOMIC_ENERGIES])
        for name, key, w64, s in zip(sc.READOUT_OUTPUTS, keys, want, scales):
            w_.add(name, out[key], w64, s.s)
        if N:
            held = scales[2].s > 0                                  # the structures that hold atoms
            assert rel_err(out[K.SCALED_ATOMIC_ENERGIES], torch.tensor(want[0])) < 1e-5
            assert float((np.abs(_np64(out[K.TOTAL_ENERGY]) - want[2])[held] / np.abs(want[2])[held]).max()) < 1e-5
        empty = np.bincount(np.asarray(case["batch"]), minlength=S) == 0
        assert not _np64(out[K.SCALED_TOTAL_ENERGY])[empty].any() and not _np64(out[K.TOTAL_ENERGY])[empty].any()
    w_.record(f"readout D {D} N {N} S {S} scale {energy_scale:g}")


# ------------------------------------------------------------------------------------------------------ the index refusals
def _refuse_entry(monkeypatch, entry):
    """Replace `entry` by a counter that never reaches the device: whatever the wrapper lets through is counted, not run."""
    from torch_m3gnet import _lib

    calls = []
    monkeypatch.setattr(_lib.load_library(), entry, lambda *args: calls.append(entry) or 0)
    return calls


@pytest.mark.parametrize("key,where,value", [("triplet_edge_index", (0, 3), "E"), ("triplet_edge_index", (1, 0), -1), ("edge_index", (1, 5), "N"),
                                             ("edge_index", (0, 0), -2), ("triplet_edge_index", (1, 7), 2**33)])
def test_three_body_refuses_an_index_out_of_range_before_any_launch(key, where, value, monkeypatch):
    """m3g_three_body indexes with the caller's lists as they are: ThreeBodyInteration.forward raises the fused path's ValueError first.
    (The entry point is replaced by a counter here, so that no kernel could see such an index even if the check were missing.)"""
    case = sc.three_body_case(3, 3, 64)
    mod, inputs = _three_body(case)
    inputs[key] = inputs[key].clone()
    inputs[key][where] = {"E": case["dist"].shape[0], "N": 20}.get(value, value)
    calls = _refuse_entry(monkeypatch, "m3g_three_body")
    with pytest.raises(ValueError, match="out of range"):
        mod(dict(inputs))
    assert calls == []


def test_three_body_rechecks_a_list_changed_in_place_after_its_topology_was_built(monkeypatch):
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.modules import _Topology

    case = sc.conv_case(24, 3)
    tb = sc.three_body_case(3, 3, 64)
    _, graph = _conv(case)
    _Topology.of(graph)                                              # a valid graph: its lists are range-checked by the build
    calls = _refuse_entry(monkeypatch, "m3g_three_body")
    mod, _ = _three_body(tb)
    E, T = case["e"].shape[0], case["graph"]["triplet_edge_index"].shape[1]
    rng = np.random.default_rng(0)
    graph.update({K.NODE_FEATURES: _d(rng.normal(0, 1, (65, 64)).astype(np.float32)), K.EDGE_ATTR: _d(rng.normal(0, 1, (E, 64)).astype(np.float32)),
                  K.EDGE_DISTANCES: torch.full((E,), 2.0, device=DEV), K.TRIPLET_ANGLES: torch.zeros(T, device=DEV)})
    mod(graph)
    assert calls == ["m3g_three_body"]                               # accepted on the strength of the cached topology
    graph[K.TRIPLET_EDGE_INDEX][0, 0] = E                            # in place: the cache no longer vouches for the list
    with pytest.raises(ValueError, match="out of range"):
        mod(graph)
    assert calls == ["m3g_three_body"]


@pytest.mark.parametrize("where,value", [(4, "S"), (0, -1), (64, 2**40)])
def test_readout_refuses_a_batch_out_of_range_before_any_launch(where, value, monkeypatch):
    from torch_m3gnet.data import MaterialGraphKey as K

    mod, inputs = _readout(sc.readout_case(64, 65, 4, 1.0))
    inputs[K.BATCH] = inputs[K.BATCH].clone()
    inputs[K.BATCH][where] = 4 if value == "S" else value
    calls = _refuse_entry(monkeypatch, "m3g_readout")
    with pytest.raises(ValueError, match="out of range"):
        mod(dict(inputs))
    assert calls == []


def test_three_body_refuses_tensors_that_do_not_fit_the_lists(monkeypatch):
    """The kernel reads E rows of edge_attr and distances, T angles and one width D for x and edge_attr: anything else is a ValueError on
    the host, before the entry point is called."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.nn.interaction import ThreeBodyInteration

    case = sc.three_body_case(3, 3, 64)
    mod, inputs = _three_body(case)
    calls = _refuse_entry(monkeypatch, "m3g_three_body")
    for key, wrong in ((K.EDGE_ATTR, inputs[K.EDGE_ATTR][:-1]), (K.EDGE_ATTR, inputs[K.EDGE_ATTR][:, :-1]), (K.EDGE_DISTANCES, inputs[K.EDGE_DISTANCES][:-1]),
                       (K.TRIPLET_ANGLES, inputs[K.TRIPLET_ANGLES][1:]), (K.NODE_FEATURES, inputs[K.NODE_FEATURES][:, :32])):
        with pytest.raises(ValueError):
            mod(dict(inputs, **{key: wrong.contiguous()}))
    uneven = ThreeBodyInteration(5.0, 4.0, 3, 3, 64, 32).to(DEV)      # num_edge_features != num_node_features: m3g_three_body has one width
    with pytest.raises(ValueError, match="num_node_features = num_edge_features"):
        uneven(dict(inputs, **{K.EDGE_ATTR: inputs[K.EDGE_ATTR][:, :32].contiguous()}))
    assert calls == []
    mod(dict(inputs))
    assert calls == ["m3g_three_body"]                                # (the untouched inputs pass)


def test_readout_refuses_tensors_that_do_not_fit_the_atoms(monkeypatch):
    from torch_m3gnet.data import MaterialGraphKey as K

    mod, inputs = _readout(sc.readout_case(64, 65, 4, 1.0))
    calls = _refuse_entry(monkeypatch, "m3g_readout")
    for key, wrong in ((K.ELEMENTAL_ENERGIES, inputs[K.ELEMENTAL_ENERGIES][:-1]), (K.BATCH, inputs[K.BATCH][:-1]), (K.NODE_FEATURES, inputs[K.NODE_FEATURES][:, :32])):
        with pytest.raises(ValueError):
            mod(dict(inputs, **{key: wrong.contiguous()}))
    assert calls == []
    mod(dict(inputs))
    assert calls == ["m3g_readout"]
