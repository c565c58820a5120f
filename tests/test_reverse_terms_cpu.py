"""CPU audit of tests/reverse_term_cases.py: how much of max|F| every term of the hand-derived reverse pass carries on the inputs that
tests/test_gpu_reverse_terms.py runs, from the fp64 staged oracle alone (oracle/staged.py: forward_backward(ablate=...), term_shares).

A force gate of 1e-4 of max|F| holds a term of share s to 1e-4 / s of itself: at s >= 0.03 to 0.33 % or better, at the 1e-5 .. 1e-3 the
three-body and gate-derivative terms have with freshly initialised weights not at all.

Share condition: every term >= 0.03 on at least one configuration of each kernel selection; angular_t2, tb_basis and dm >= 0.03 on each
of the one-sided / thinned / asymmetric / dense inputs.  Headroom condition: the fp32 CPU oracle is at least 10 x inside every gate of
the GPU tests (E 1e-5, F 1e-4, stress 1e-4, mid_edge_features 1e-4) on every configuration, so a device result near a gate is the
kernels' doing and not the arithmetic's.

Measured (fp64 staged oracle; fp32 CPU oracle against the fp64 oracle, 8 threads), weighted models:

  shape   input       cutoff basis  angular  t1     t2     u-proj atom   dm     dense  gate   TA     TB     dh_conv dh_emb de_e   de_n  | fp32: E       F       stress  m
  default cells18     0.226  0.171  0.133  0.088  0.064  0.133  0.177  0.367  0.307  0.120  0.058  0.058  1.108   0.072  0.055  0.368 | 1.6e-7  1.5e-6  2.9e-6  3.1e-6
  tbs1    cells18     0.188  0.304  0.130  0.041  0.115  0.053  0.059  0.344  0.351  0.091  0.058  0.055  0.731   0.060  0.050  0.345 | 1.2e-7  2.0e-6  9.5e-7  2.8e-6
  tbs2    cells18     0.157  0.304  0.068  0.046  0.047  0.052  0.159  0.379  0.305  0.132  0.104  0.072  0.813   0.098  0.072  0.453 | 5.4e-8  1.6e-6  2.8e-6  2.7e-6
  tbs3    cells18     0.158  0.166  0.130  0.067  0.096  0.119  0.129  0.270  0.207  0.121  0.055  0.066  0.957   0.138  0.073  0.287 | 1.1e-7  2.7e-6  1.3e-6  3.1e-6
  tbs4    cells18     0.167  0.384  0.169  0.111  0.096  0.196  0.063  0.451  0.375  0.131  0.051  0.071  1.182   0.134  0.099  0.509 | 5.4e-8  2.1e-6  8.9e-7  2.6e-6
  any96   cells18     0.276  0.550  0.178  0.111  0.149  0.148  0.164  0.617  0.495  0.227  0.085  0.108  0.791   0.146  0.145  0.718 | 7.6e-8  1.9e-6  2.5e-6  2.5e-6
  default one_sided   0.453  0.596  0.248  0.088  0.159  0.342  0.196  0.548  0.495  0.086  0.091  0.080  0.858   0.102  0.107  0.706 | 4.4e-8  2.1e-6  1.3e-6  3.3e-6
  default thinned     0.258  0.314  0.156  0.097  0.173  0.297  0.073  0.360  0.334  0.059  0.078  0.113  1.113   0.137  0.034  0.366 | 6.2e-8  2.0e-6  2.3e-6  1.7e-6
  default asymmetric  0.230  0.338  0.152  0.117  0.093  0.184  0.192  0.480  0.413  0.083  0.044  0.064  0.935   0.050  0.050  0.504 | 9.1e-8  1.2e-6  3.0e-6  1.8e-6
  dense   dense       0.230  0.200  0.232  0.080  0.162  0.390  0.956  1.163  0.908  0.249  0.360  0.281  0.753   0.076  0.222  1.222 | 1.9e-7  3.9e-6  3.2e-6  2.6e-6
  (default / any96 on fcc32: the table of test_configuration_meets_the_share_and_headroom_conditions' docstring)

The same shapes with the weights as initialised (what the suite ran these inputs on before): default / cells18 tb_cutoff 1.4e-3, tb_basis
1.8e-3, angular 1.2e-3, angular_t2 9.8e-4, dm 2.5e-3, atom_gate 3.7e-6, dm_gate 1.7e-5, de_edge 3.2e-5 -- test_fresh_weights_leave_the_three_body_terms_below_the_gate pins that this
is what the scaling cures."""
import pytest
import torch

import reverse_term_cases as rc
from helpers import rel_err
from oracle import m3gnet_oracle as orc, staged

SHARE_MIN = 0.03
GATES = dict(e=1e-5, f=1e-4, s=1e-4, m=1e-4)   # the fp32 / f16x3 gates of tests/test_gpu_reverse_terms.py (bf16x3's are wider)
HEADROOM = 10.0
FORWARD_KEYS = ("total_energy", "scaled_atomic_energies", "x", "edge_attr", "m_0", "e1_0", "e2_0", "x_0", "q", "qp", "h", "hp", "dx_readout")


@pytest.fixture(scope="module")
def default_case():
    torch.set_num_threads(8)
    args = rc.oracle_inputs(rc.shape_model("default", "cells18"), rc.input_batch("cells18"))
    return args, staged.forward_backward(*args)


def _forces_without(args, *names):
    return staged.forward_backward(*args, ablate=set(names))["forces"]


def test_no_switch_set_changes_no_bit_and_unknown_names_are_refused(default_case):
    args, full = default_case
    again = staged.forward_backward(*args, ablate=frozenset())
    assert full.keys() == again.keys()
    for k in full:
        assert torch.equal(full[k], again[k]), k
    with pytest.raises(ValueError):
        staged.forward_backward(*args, ablate={"angular_t3"})


@pytest.mark.parametrize("term", list(staged.REVERSE_TERMS))
def test_each_switch_changes_the_forces_and_nothing_forward(default_case, term):
    args, full = default_case
    off = staged.forward_backward(*args, ablate={term})
    for k in FORWARD_KEYS:
        assert torch.equal(off[k], full[k]), (term, k)
    assert float((off["forces"] - full["forces"]).abs().max()) > 1e-3 * float(full["forces"].abs().max()), term
    assert not torch.equal(off["stresses"], full["stresses"]), term


def _linear_in_halves(args, full, whole, halves):
    f = full["forces"]
    d_whole = f - _forces_without(args, whole)
    d_halves = sum(f - _forces_without(args, half) for half in halves)
    assert float(d_whole.abs().max()) > SHARE_MIN * float(f.abs().max())
    assert float((d_whole - d_halves).abs().max()) < 1e-12 * float(f.abs().max())
    assert torch.equal(_forces_without(args, *halves), _forces_without(args, whole))


def test_the_angular_term_is_the_sum_of_its_halves(default_case):
    """F - F_without(angular) = sum over t1, t2 of F - F_without(half), to fp64 rounding (d_u goes straight to the geometry reverse, so
    this holds with any number of blocks); and both halves off is the whole off, bit for bit."""
    _linear_in_halves(*default_case, "angular", ("angular_t1", "angular_t2"))


def test_d_m_is_the_sum_of_its_halves_in_a_block():
    """The same for d_m = MM(d_pd, wd) + MM(d_pg, wg) -- in a ONE-block model.  A switch acts in every block, and d_m of block b reaches
    d_m of block b - 1 through d_v and d_x, so with several blocks the halves' differences hold cross terms (dense half of one block
    times gate half of another: 3.5 % of max|F| on the default shape) and do not add up to the whole's."""
    torch.set_num_threads(8)
    args = rc.oracle_inputs(rc.weighted_model(3, 3, 64, 1, 5.0, 4.0), rc.input_batch("cells18"))
    _linear_in_halves(args, staged.forward_backward(*args), "dm", ("dm_dense", "dm_gate"))


def test_term_shares_is_the_ablation_it_says(default_case):
    args, full = default_case
    sh = staged.term_shares(*args, names=("tb_cutoff", "dm"))
    for name, share in sh.items():
        assert share == float((full["forces"] - _forces_without(args, name)).abs().max()) / float(full["forces"].abs().max())
    assert set(rc.shares("default", "cells18")) == set(staged.REVERSE_TERMS)


def test_l_max_1_has_no_angular_term():
    """P_0 is constant: with l_max = 1 the three angular switches (and the u-projection, which only d_u feeds) change no bit of the
    forces, so no l_max = 1 shape is among the configurations -- it could not meet the share condition for them.  The other three-body
    terms are there as usual."""
    torch.set_num_threads(8)
    args = rc.oracle_inputs(rc.weighted_model(1, 3, 64, 2, 5.0, 4.0), rc.input_batch("cells18"))
    sh = staged.term_shares(*args)
    for name in ("angular", "angular_t1", "angular_t2", "du_projection"):
        assert sh[name] == 0.0, (name, sh[name])
    assert all(l_max > 1 for l_max, *_ in rc.SHAPES.values())
    assert min(sh["tb_cutoff"], sh["tb_basis"], sh["dm"]) > SHARE_MIN, sh


def test_fresh_weights_leave_the_three_body_terms_below_the_gate():
    """What the weighted models are for: as initialised, the default shape on the random cells gives the atom-gate reverse and the gate
    half of d_m less than the 1e-4 force gate itself, and every three-body term less than 0.3 % of max|F|."""
    sh = rc.shares("default", "cells18", weighted=False)
    assert sh["atom_gate"] < 1e-4 and sh["dm_gate"] < 1e-4, sh
    assert max(sh[k] for k in ("tb_cutoff", "tb_basis", "angular", "angular_t1", "angular_t2", "dm")) < 3e-3, sh
    weighted = rc.shares("default", "cells18")
    assert min(weighted.values()) >= SHARE_MIN, weighted


@pytest.mark.parametrize("shape,name", rc.CONFIGURATIONS)
def test_configuration_meets_the_share_and_headroom_conditions(shape, name):
    """Per configuration: the staged reverse equals autograd (fp64, 1e-10: also on the fcc cell, where 48 triplets have |cos| > 1 in
    fp64 and the clamp's `inside` factor is 0), the three-body terms carry >= 3 % each, the list inputs give angular_t2, tb_basis and
    dm >= 3 %, and the fp32 CPU oracle is >= 10 x inside every fp32 gate.

    The perfect fcc cell (lattice constant 2.8 A: 54 partners per centre, 91,584 triplets, of which 3,264 collinear -- |cos| within
    1e-12 of 1, 376 exactly 1, 48 beyond):
      default fcc32  cutoff 0.334  basis 1.053  angular 0.326  t1 0.332  t2 0.116  smallest de_edge 0.086 | fp32: E 1.3e-7  F 5.7e-6  stress 5.7e-6  m 1.8e-6
      any96   fcc32  cutoff 0.432  basis 0.951  angular 0.191  t1 0.108  t2 0.119  smallest de_edge 0.063 | fp32: E 1.2e-7  F 6.1e-6  stress 1.9e-6  m 1.1e-6"""
    torch.set_num_threads(8)
    model, batch = rc.shape_model(shape, name), rc.input_batch(name)
    o = rc.oracle64(shape, name)
    st = staged.forward_backward(*rc.oracle_inputs(model, batch))
    assert rel_err(st["forces"], o["forces"]) < 1e-10 and rel_err(st["stresses"], o["stresses"]) < 1e-10
    sh = rc.shares(shape, name)
    print(f"{shape} {name}: max|F| {float(o['forces'].abs().max()):.3g}  " + "  ".join(f"{k} {v:.3f}" for k, v in sh.items()))
    for term in ("tb_cutoff", "tb_basis", "angular", "angular_t1", "angular_t2", "dm", "dm_dense", "dm_gate", "atom_gate"):
        assert sh[term] >= SHARE_MIN, (term, sh[term])
    if name in rc.LIST_INPUTS:
        assert min(sh["angular_t2"], sh["tb_basis"], sh["dm"]) >= SHARE_MIN, sh
    # headroom: the reference's own fp32 arithmetic on this configuration
    p, cfg, c, og = rc.oracle_inputs(model, batch, dtype=torch.float32)
    o32 = orc.energy_forces(p, cfg, c, og, legendre_backward="exact")
    err = dict(e=float(((o32["total_energy"].double() - o["total_energy"]).abs() / o["total_energy"].abs()).max()),
               f=rel_err(o32["forces"], o["forces"]), s=rel_err(o32["stresses"], o["stresses"]),
               m=max(rel_err(o32[f"mid_edge_features_{b}"], o[f"mid_edge_features_{b}"]) for b in range(cfg.num_blocks)))
    print("   fp32 CPU oracle against fp64: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, gate in GATES.items():
        assert err[k] * HEADROOM <= gate, (k, err[k], gate)


@pytest.mark.parametrize("selection", list(rc.SELECTIONS))
def test_every_selection_runs_every_term_at_three_percent_somewhere(selection):
    """The share condition per kernel selection: over the configurations a selection runs, every named term reaches >= 3 %."""
    configs = rc.SELECTION_CONFIGS[selection]
    best = {term: max(rc.shares(shape, name)[term] for shape, name in configs) for term in staged.REVERSE_TERMS}
    assert min(best.values()) >= SHARE_MIN, {k: v for k, v in best.items() if v < SHARE_MIN}


def test_the_fcc_cell_has_collinear_triplets_of_both_signs():
    """cos = -1 (across the centre) and cos = +1 (two neighbours along one close-packed row) both occur, thousands of times; in fp64
    some land beyond 1, so the oracle's clamp fires -- no other input of the suite has such a triplet."""
    args = rc.oracle_inputs(rc.shape_model("default", "fcc32"), rc.input_batch("fcc32"))
    st = staged.forward_backward(*args)
    tei = args[3]["triplet_edge_index"]
    cos = (st["u"][tei[0]] * st["u"][tei[1]]).sum(1)
    assert int((cos > 1 - 1e-12).sum()) > 500 and int((cos < -1 + 1e-12).sum()) > 500
    assert int((cos.abs() > 1).sum()) > 0
    assert int(rc.input_batch("fcc32")["pos"].shape[0]) == 32
