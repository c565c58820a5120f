"""GPU: the stamped diagnostic variants of the edge kernels (plan option "stamps": 1 forward kernel, 2 edge-MLP kernel of the reverse
pair, 3 fused reverse kernel; tools/stamp_report*.py) are the shipped kernels plus s_memtime reads: they must leave energies, forces
and stresses bit-identical, and every wave that worked must have written non-zero phase sums."""
import numpy as np
import pytest
import torch

from helpers import fcc_cu_graph

pytestmark = pytest.mark.gpu

# target -> (precision, options under which the target's stamped kernel is the one that runs (resolve_step_path and the launchers:
# 1 any precision, 2 bf16x3 and the kernel pair, 3 f16x3 and the fused kernel), waves per workgroup, phase marks the kernel passes)
STAMPED = {
    1: ("f16x3", {}, 12, (0, 1, 2, 3, 5, 6, 7, 8, 10, 11)),   # k_edge_block_mfma: marks 0, 1, 6, 11 + {0, 1, 3} past 2 and 7 per MLP
    2: ("bf16x3", {"rev_kernel": 0}, 12, (1, 2, 3, 4, 5, 6, 7)),   # k_edge_rev_edge_mlp
    3: ("f16x3", {}, 8, tuple(range(12))),   # k_edge_rev_fused
}


@pytest.mark.parametrize("target", sorted(STAMPED))
def test_stamped_fused_reverse_is_bit_identical_and_writes_stamps(target):
    from torch_m3gnet import _lib
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.model.build import build_model

    precision, options, waves, marks = STAMPED[target]
    torch.manual_seed(0)
    model = build_model(5.0, 4.0, 3, 3, 95, 64, 3).cuda()
    eng = model.engine
    eng.set_precision(precision)
    for name, value in options.items():
        eng.set_option(name, value)
    g = fcc_cu_graph(4, 4, 6).to("cuda")
    out = model(g)
    ref = {k: out[k].clone() for k in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)}
    eng.set_option("stamps", target)
    try:
        out = model(g)
        torch.cuda.synchronize()
        for k, v in ref.items():
            assert torch.equal(out[k], v), k
        buf = np.zeros(256 * 16 * 12, dtype=np.uint64)
        _lib.check(eng.lib.m3g_debug_read_stamps(eng.plan, buf.ctypes.data))
        s = buf.reshape(256, 16, 12)
        unused = [i for i in range(12) if i not in marks]
        assert s[:, :waves].sum() > 0 and s[:, waves:].sum() == 0 and s[:, :, unused].sum() == 0
        busy = s[:, :waves].sum(-1) > 0
        assert busy.any() and (s[:, :waves][busy][:, list(marks)] > 0).all()    # a wave that processed a tile passed every phase mark
    finally:
        eng.set_option("stamps", 0)
    out = model(g)
    for k, v in ref.items():
        assert torch.equal(out[k], v), k


def test_stamps_switched_on_under_graph_replay_are_not_served_the_unstamped_graph():
    """Every option is part of the key of a captured launch sequence.  With graph_replay on, switching "stamps" on between two calls on
    identical buffers must capture anew: the first call's graph holds the unstamped kernel and no stamp buffer, and replaying it leaves
    the buffer at zero.  The stamped kernel is the shipped kernel plus s_memtime reads: same forces, bit for bit."""
    from torch_m3gnet import _lib
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(0)
    model = build_model(5.0, 4.0, 3, 3, 95, 64, 3).cuda()
    eng = model.engine
    g = fcc_cu_graph(2, 2, 2).to("cuda")
    eng.set_option("graph_replay", 1)
    try:
        eng.set_precision("f16x3")
        f0 = model(g)[K.FORCES].clone()
        eng.set_option("stamps", 3)
        f1 = model(g)[K.FORCES].clone()   # (same graph object, engine-owned outputs: the buffers of the first call)
        torch.cuda.synchronize()
        buf = np.zeros(256 * 16 * 12, dtype=np.uint64)
        _lib.check(eng.lib.m3g_debug_read_stamps(eng.plan, buf.ctypes.data))
        assert buf.any()
        assert torch.equal(f1, f0)
    finally:
        eng.set_option("stamps", 0)
        eng.set_option("graph_replay", 0)


def test_readout_f16_option_agrees_with_the_exact_readout():
    """f16x3 mode: the readout layers run on exact-fp32 chains by default; option readout_f16 = 1 moves them to scaled two-part fp16
    chains (22-24 bits per product).  On a well-conditioned cell both give the same energies and forces to fp32 rounding."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(0)
    model = build_model(5.0, 4.0, 3, 3, 95, 64, 3).cuda()
    model.engine.set_precision("f16x3")
    g = fcc_cu_graph(3, 3, 4).to("cuda")
    out = model(g)
    e0, f0 = out[K.TOTAL_ENERGY].clone(), out[K.FORCES].clone()
    model.engine.set_option("readout_f16", 1)
    try:
        out = model(g)
        e1, f1 = out[K.TOTAL_ENERGY].clone(), out[K.FORCES].clone()
    finally:
        model.engine.set_option("readout_f16", 0)
    assert not torch.equal(f0, f1)   # a different kernel really ran
    assert float(((e1 - e0).abs() / e0.abs()).max()) < 2e-6
    assert float((f1 - f0).abs().max() / f0.abs().max()) < 1e-5
    out = model(g)
    assert torch.equal(out[K.FORCES], f0)


def test_launch_count_comes_from_a_capture_of_the_unprofiled_call():
    """m3g_count_launches (what bench.py reports as kernel_launches_per_step): the launch sequence of ONE m3g_energy_forces call is
    captured on a stream of the library's own -- nothing executes, no buffer is touched -- and its nodes are counted.  The counted call
    and the calls around it return identical bits; the 32-atom cell takes the 17 launches of DESIGN.md section 2a, an energy-only call
    fewer, and the stage profiler (which runs a slightly different sequence) does not disturb the count."""
    import torch

    from helpers import build_engine_model, engine_graph, load_oracle_case
    from torch_m3gnet.data import MaterialGraphKey as K

    model, _ = build_engine_model("cu32fit", "doc")
    model.engine.set_precision("fp32")   # (the count below is the exact-fp32 sequence's, whatever M3G_PRECISION says)
    _, _, _, graph, _ = load_oracle_case("cu32fit", "doc")
    g = engine_graph(graph)
    before = {k: model(g, extras=False)[k].clone() for k in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES)}
    kernels, other = model.engine.count_launches(lambda: model(g, extras=False))
    during = {k: g[k].clone() for k in before}
    after = {k: model(g, extras=False)[k].clone() for k in before}
    for k in before:
        assert torch.equal(before[k], during[k]) and torch.equal(before[k], after[k]), k
    assert kernels == 17 and other == 0, (kernels, other)
    k_energy, _ = model.engine.count_launches(lambda: model(g, forces=False, extras=False))
    assert 0 < k_energy < kernels
    model.engine.profile(True)
    try:
        assert model.engine.count_launches(lambda: model(g, extras=False)) == (kernels, other)
    finally:
        model.engine.profile(False)
