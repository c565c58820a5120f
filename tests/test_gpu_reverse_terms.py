"""Every reverse-pass term of the force kernels against the fp64 oracle, on models where each term carries weight.

The gates of the suite are relative to max|F| (1e-4), so a term of the hand-derived reverse pass (B4 edge block, B3 three-body, B2 node,
B1 edge embedding, B0 geometry) is held only as tightly as its share of max|F| allows -- and with freshly initialised weights the
three-body cutoff / basis / angular terms carry ~1e-3, the atom-gate reverse and the gate half of d_m ~1e-5: they could be missing or
have the wrong sign and every other test would pass.  Here the weight groups are scaled (tests/reverse_term_cases.py) so that every term
of oracle/staged.py's REVERSE_TERMS carries >= 3 % of max|F| (>= 5 % on the default shape; audited on the CPU, with the fp32 CPU
oracle >= 10 x inside every gate, by tests/test_reverse_terms_cpu.py): the unchanged 1e-4 gate then holds each term to 0.33 % of itself or
better.  Inputs: two random 18-atom cells; a perfect fcc cell (collinear triplets, cos = +-1 exactly, |cos| > 1 after rounding);
one-sided, thinned and asymmetric lists and the dense cell of the list tests of tests/test_gpu_properties.py.  Each on every kernel
selection whose reverse is an implementation of its own (reverse_term_cases.SELECTIONS), one engine evaluation of <= 40 atoms against
one cached fp64 oracle evaluation.

Gates (unchanged: tests/test_gpu_persistent_path.py GATES): E 1e-5, F 1e-4, stress 1e-4 for fp32 and f16x3, bf16x3 E 1e-3, F 5e-4,
stress 2e-3; mid_edge_features 1e-4 (recorded, not gated, in the bf16x3 mode, as everywhere in the suite).
Measured: profiles/reverse_terms.txt."""
import functools

import pytest
import torch

import reverse_term_cases as rc
from helpers import persistent_tile_counts, record_line, rel_err, set_options, split_tail_runs
from test_gpu_persistent_path import GATES, _errors, _fmt, _keys, _outputs, _two_selections

pytestmark = pytest.mark.gpu

RECORD = "reverse_terms.txt"


@functools.lru_cache(maxsize=None)
def _run(selection, shape, name):
    """One engine evaluation of a configuration under a selection (kept: the relations between selections read it again)."""
    precision, options = rc.SELECTIONS[selection]
    model = rc.shape_model(shape, name)
    model.engine.set_precision(precision)
    if shape == "any96":
        assert options.get("edge_kernel") == 2, "width 96 is beyond every path but the any-size one"
    return _outputs(set_options(model, **options), rc.input_batch(name).clone().to("cuda"))


def _blocks(shape):
    return rc.SHAPES[shape][3]


@pytest.mark.parametrize("selection,shape,name", rc.GPU_CASES)
def test_selection_against_the_fp64_oracle(selection, shape, name):
    """E, F, stress and mid_edge_features of (selection, shape, input) inside the suite's gates.  The list inputs keep what their tests
    in tests/test_gpu_properties.py assert with the default weights: mid_edge_features 1e-4 per block (one-sided, thinned), node
    features 1e-5 (asymmetric)."""
    precision = rc.SELECTIONS[selection][0]
    err = _errors(_run(selection, shape, name), rc.oracle64(shape, name), _blocks(shape))
    record_line(RECORD, f"{shape} {name} {selection}: {_fmt(err)}")
    gate = GATES[precision]
    assert err["e"] < gate["e"] and err["f"] < gate["f"] and err["s"] < gate["s"], err
    if precision != "bf16x3":
        assert err["m"] < 1e-4, err
        if name == "asymmetric":
            assert err["x"] < 1e-5, err


TBS_ROWS = ("tbs1", "tbs2", "tbs3", "tbs4")


@pytest.mark.parametrize("selection,shape", [("persistent", shape) for shape in ("default",) + TBS_ROWS] + [("rev_saved_p1", "default")])
def test_another_fused_reverse_kernel_really_ran(selection, shape):
    """k_edge_rev_f32 with and without the saved layer-2 pre-activations against the default selection (k_edge_rev_split): forward
    outputs bit for bit, forces and stresses within 1e-5 and NOT equal -- each of these kernels associates dL/dh and dL/dm
    differently, so equal forces would mean it never ran."""
    f_diff, s_diff = _two_selections(_run("default", shape, "cells18"), _run(selection, shape, "cells18"))
    record_line(RECORD, f"{shape} cells18 {selection} vs default selection: forward bit-identical, F {f_diff:.2e}  stress {s_diff:.2e}")
    assert 0.0 < f_diff < 1e-5 and s_diff < 1e-5, (f_diff, s_diff)


@pytest.mark.parametrize("selection,shape", [(sel, "default") for sel in ("persistent_pair", "rev_recompute", "pair_saved_p1")]
                         + [("persistent_pair", shape) for shape in TBS_ROWS])
def test_the_reverse_kernel_pair_really_ran(selection, shape):
    """The node-MLP + edge-MLP kernel pair against the default selection.  Without a fused reverse kernel the step also takes another
    forward sequence (StepPath::fused_rev, csrc/m3g_step_path.h), so the forward outputs are close, not equal: energies within 1e-6
    (test_fused_and_split_reverse_kernels_agree), forces and stresses within 1e-5 and not equal."""
    K, _, _ = _keys()
    a, b = _run("default", shape, "cells18"), _run(selection, shape, "cells18")
    e_diff = float(((a[K.TOTAL_ENERGY] - b[K.TOTAL_ENERGY]).abs() / a[K.TOTAL_ENERGY].abs()).max())
    f_diff, s_diff = rel_err(b[K.FORCES], a[K.FORCES]), rel_err(b[K.STRESSES], a[K.STRESSES])
    record_line(RECORD, f"{shape} cells18 {selection} vs default selection: E {e_diff:.2e}  F {f_diff:.2e}  stress {s_diff:.2e}")
    assert e_diff < 1e-6 and 0.0 < f_diff < 1e-5 and s_diff < 1e-5, (e_diff, f_diff, s_diff)


def test_split_tail_of_the_persistent_reverse_kernel_really_ran():
    """Every workgroup of these inputs has one tile or none (asserted), which split_tail = 1 takes out of the whole-tile body of
    k_edge_rev_f32: against split_tail = 0 forward bit for bit, forces within 1e-5 and not equal."""
    K, _, _ = _keys()
    counts = persistent_tile_counts(int(rc.input_batch("cells18")[K.EDGE_INDEX].shape[1]))
    assert max(counts) == 1 and split_tail_runs(counts, 1) and not split_tail_runs(counts, 0), counts
    f_diff, s_diff = _two_selections(_run("persistent", "default", "cells18"), _run("persistent_tail", "default", "cells18"))
    record_line(RECORD, f"default cells18 persistent_tail vs persistent: forward bit-identical, F {f_diff:.2e}  stress {s_diff:.2e}")
    assert 0.0 < f_diff < 1e-5 and s_diff < 1e-5, (f_diff, s_diff)


def test_recomputing_pair_is_one_path_under_either_rev_kernel():
    """save_p1 = 0 leaves the fused reverse kernels nothing to start from: rev_kernel 1 and 0 resolve to the same kernel pair
    (resolve_step_path, csrc/m3g_step_path.h) -- every output equal bit for bit."""
    a, b = _run("rev_recompute", "default", "cells18"), _run("pair_recompute", "default", "cells18")
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("shape,name", [("default", "cells18"), ("default", "fcc32"), ("default", "asymmetric")])
def test_moment_and_list_kernels_both_ran(shape, name):
    """threebody_moments 1 (default; these lists are complete) and 0 sum in different orders: bit-equal aggregates would mean the moment
    kernels never ran.  Apart by the tolerances of test_threebody_moment_and_list_paths_agree (tests/test_gpu_parity.py)."""
    K, _, _ = _keys()
    a, b = _run("default", shape, name), _run("list", shape, name)
    m_d, f_d, s_d = (rel_err(a[k], b[k]) for k in (K.MID_EDGE_FEATURES, K.FORCES, K.STRESSES))
    record_line(RECORD, f"{shape} {name} moment vs list kernels: mid_edge_features {m_d:.2e}  F {f_d:.2e}  stress {s_d:.2e}")
    assert not torch.equal(a[K.MID_EDGE_FEATURES], b[K.MID_EDGE_FEATURES]), "the moment path did not run"
    assert m_d < 5e-6 and f_d < 1e-5 and s_d < 1e-5, (m_d, f_d, s_d)


def test_which_inputs_the_moment_kernels_may_take():
    """The topology's certificate (m3g_topology_hints bit 0: every partner list complete, windows within the moment kernels' LDS) is
    set for the random cells, the fcc cell and the asymmetric edge list (whose triplets are all pairs of the edges that remain) and NOT
    for the one-sided and thinned triplet lists (incomplete) nor for the dense cell (~100 partners per centre: its windows are too
    large) -- those run the list kernels under the default selection."""
    from torch_m3gnet.nn.modules import _Topology

    hints = {name: _Topology(rc.input_batch(name).clone().to("cuda")).query_hints() & 1 for name in rc.INPUTS}
    assert hints == dict(cells18=1, fcc32=1, one_sided=0, thinned=0, asymmetric=1, dense=0), hints


def test_node_and_threebody_reverse_in_one_launch_and_in_two():
    """fuse_node_tb 1 (default; <= 128 atoms, moment path) and 0 give the same bits (test_node_and_threebody_reverse_in_one_launch_is_
    bit_identical) -- so that both really ran is read off the launch counts: one launch more per block after the first."""
    K, _, _ = _keys()
    a, b = _run("default", "default", "cells18"), _run("two_launches", "default", "cells18")
    for k in a:
        assert torch.equal(a[k], b[k]), k
    counts = {}
    for fused in (1, 0):
        model = set_options(rc.shape_model("default", "cells18"), fuse_node_tb=fused)
        g = rc.input_batch("cells18").clone().to("cuda")
        model(g, extras=False)
        counts[fused] = model.engine.count_launches(lambda: model(g, extras=False))[0]
    record_line(RECORD, f"default cells18 kernel launches per step: fuse_node_tb 1: {counts[1]}, 0: {counts[0]}")
    assert counts[0] == counts[1] + _blocks("default") - 1, counts
