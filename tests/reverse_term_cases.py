"""Models and inputs on which every term of the hand-derived reverse pass carries weight (checker plumbing, CPU only).

The force gate of the suite is 1e-4 of max|F|, so a reverse term is held only as tightly as its share of max|F| allows
(oracle/staged.py: REVERSE_TERMS, term_shares).  With freshly initialised weights the three-body terms carry 1e-3 of max|F| or less and
the two sigmoid-gate derivatives 1e-4 or less.  `weighted_model` scales the weight groups of the seeded construction the suite uses so
that each term carries at least 3 % (audited by tests/test_reverse_terms_cpu.py, run on the device by tests/test_gpu_reverse_terms.py);
the inputs are the smallest that reach each branch of the three-body kernels, and the list variants are the constructions of
test_one_sided_and_filtered_triplet_lists, test_asymmetric_edge_lists_take_the_sorted_incoming_lists and
test_dense_three_body_rows_beyond_the_staged_window (tests/test_gpu_properties.py), which take them from here."""
from __future__ import annotations

import functools

import numpy as np
import torch

from helpers import PERSISTENT, PERSISTENT_TAIL, random_cell_graph
from oracle import m3gnet_oracle as orc, staged

# name -> (l_max, n_max, width, blocks, cutoff, three-body cutoff).  C = l_max * n_max channels: 4, 8, 12, 16 are the four three-body
# slab counts (TBS = 1 .. 4) of the MFMA edge kernels; width 96 is beyond their tiles, so only the any-size path (edge_kernel = 2) runs it.
SHAPES = {
    "default": (3, 3, 64, 3, 5.0, 4.0),
    "tbs1": (2, 2, 64, 2, 5.0, 4.0),
    "tbs2": (2, 4, 64, 2, 5.0, 4.0),
    "tbs3": (3, 4, 64, 2, 5.0, 4.0),
    "tbs4": (4, 4, 64, 2, 5.0, 4.0),
    "any96": (3, 3, 96, 2, 5.0, 4.0),
    "dense": (3, 3, 64, 3, 5.0, 5.0),    # the default shape under the dense cell's three-body cutoff
}
MFMA_SHAPES = ("default", "tbs1", "tbs2", "tbs3", "tbs4")

# Per-group factors on the seeded initialisation (found by a few minutes of search on the CPU, not claimed optimal): the three-body
# gated update x 100 takes W m out of the linear part of SiLU and of the sigmoid, the atom gate's Linear x 30 takes v off 1/2, and
# everything else x 3 / biases x 2 is the "trained-like" scaling of tests/test_gpu_parity.py (_scaled_like_trained), a little milder;
# the conv edge MLP x 5 brings its share of d_e (de_edge) from 1.5 % to 5.5 %.
SCALES = dict(threebody=100.0, atom_gate=30.0, edge_mlp=5.0, other=3.0, bias=2.0)
# The perfect fcc cell and the dense cell have 54 and ~100 three-body partners per centre against ~19 in the random cells, so m is that
# much larger: with x 100 the fp32 CPU oracle itself is less than 10 x inside the force / stress gates there, with x 25 (and, on the fcc cell, the
# edge MLP x 4) it is 15 x or more.
INPUT_SCALES = {"fcc32": dict(SCALES, threebody=25.0, edge_mlp=4.0), "dense": dict(SCALES, threebody=25.0)}


def weighted_model(l_max, n_max, dim, blocks, cutoff, tb_cutoff, seed=0, num_types=95, scales=SCALES):
    """The suite's seeded model (documented chi factors) with elemental energies of ONE sign -- with the sweep's -1 .. 1 the total is a
    remainder of cancelling terms and the fp32 reference itself misses 1e-5 on E -- and its weight groups scaled by `scales`
    (None: left as initialised)."""
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(seed)
    model = build_model(cutoff, tb_cutoff, l_max, n_max, num_types, dim, blocks, elemental_energies=torch.linspace(-3.0, -1.0, num_types),
                        energy_scale=2.0)
    for m in model.model:
        if type(m).__name__ == "ThreeBodyInteration":
            m.nsb.factors = m.nsb.documented_factors()
    if scales is not None:
        with torch.no_grad():
            for name, p in model.model.named_parameters():
                if name.endswith("bias"):
                    p.mul_(scales["bias"])
                elif ".gated_mlp." in name:
                    p.mul_(scales["threebody"])
                elif ".linear_sigmoid1." in name:
                    p.mul_(scales["atom_gate"])
                elif ".concat_edge_update." in name:
                    p.mul_(scales.get("edge_mlp", scales["other"]))
                else:
                    p.mul_(scales["other"])
    return model


def shape_model(shape: str, name: str, weighted=True):
    """The model of configuration (shape, input name)."""
    return weighted_model(*SHAPES[shape], scales=INPUT_SCALES.get(name, SCALES) if weighted else None)


# ------------------------------------------------------------------ inputs
def _K():
    from torch_m3gnet.data import MaterialGraphKey as K

    return K


def cells18(cutoff=5.0, tb_cutoff=4.0):
    """(a) the two random 18-atom cells of test_bare_sequential_matches_the_fused_call_and_the_oracle."""
    from torch_m3gnet.data.material_graph import Batch

    return Batch.from_data_list([random_cell_graph(18, 6.2, s, cutoff=cutoff, tb_cutoff=tb_cutoff) for s in (4, 5)])


FCC_A = 2.8   # A: nearest neighbours at 1.98 and, along the same close-packed row, 3.96 < 4.0 -- so cos = +1 occurs as well as -1


def fcc32(cutoff=5.0, tb_cutoff=4.0):
    """(b) a perfect 2 x 2 x 2 fcc cell, 32 atoms, random species, no jitter: every atom has exactly collinear triplets (cos = -1 across
    it and, with this lattice constant, cos = +1 along a row), where |dY/dcos| is largest, a reverse through the angle instead of the
    cosine is singular and the clamp of the cosine may fire in fp32."""
    from torch_m3gnet.data.material_graph import Batch, MaterialGraph
    from torch_m3gnet.data.synthetic import fcc_cu_arrays

    lat, pos, _ = fcc_cu_arrays(2, 2, 2, a=FCC_A, jitter=0.0)
    z = np.random.default_rng(5).integers(1, 95, len(pos))
    return Batch.from_data_list([MaterialGraph.from_arrays(lat, pos, z, cutoff, tb_cutoff)])


def triplet_list_variants():
    """(c) {name: batch}: the two 20-atom cells of test_one_sided_and_filtered_triplet_lists with a one-sided (e1 < e2 only), a randomly
    thinned and a single-pair triplet list.  One-sided and thinned lists hold edges that only ever appear as the partner e2."""
    from torch_m3gnet.data.material_graph import Batch

    K = _K()
    base = Batch.from_data_list([random_cell_graph(20, 6.5, s) for s in (7, 8)])
    tei = base[K.TRIPLET_EDGE_INDEX]
    gen = torch.Generator().manual_seed(0)
    subs = {
        "one_sided": tei[:, tei[0] < tei[1]],
        "thinned": tei[:, torch.rand(tei.size(1), generator=gen) < 0.3],
        "single_pair": tei[:, :1],
    }
    out = {}
    for name, sub in subs.items():
        g = base.clone()
        g[K.TRIPLET_EDGE_INDEX] = sub.contiguous()
        g[K.NUM_TRIPLETS] = int(sub.size(1))
        out[name] = g
    return out


def edge_list_variants(tb_cutoff=4.0):
    """(c) {(cell, variant): batch}: the cells of test_asymmetric_edge_lists_take_the_sorted_incoming_lists -- a 24-atom cell with its
    symmetric edge list and with 15 % of the directed edges dropped (i -> j kept, j -> i gone), and a 5-atom multigraph cell (several
    images of the same neighbour) -- each with the triplets of the edges that remain."""
    from torch_m3gnet.data.material_graph import Batch
    from torch_m3gnet.data.neighbors import threebody_index

    K = _K()
    out = {}
    for name, cell in (("thinned", random_cell_graph(24, 7.0, 21)), ("multigraph", random_cell_graph(5, 3.9, 22, dmin=1.8))):
        base = Batch.from_data_list([cell])
        ei, shift = base[K.EDGE_INDEX], base[K.EDGE_CELL_SHIFT]
        variants = {"symmetric": torch.ones(ei.size(1), dtype=torch.bool)}
        if name == "thinned":
            variants["asymmetric"] = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(1)) < 0.85   # drops one direction of many pairs
        for vname, keep in variants.items():
            g = base.clone()
            g[K.EDGE_INDEX] = ei[:, keep].contiguous()
            g[K.EDGE_CELL_SHIFT] = shift[keep].contiguous()
            # triplets of the remaining edges (distances from the positions, as the builders form them)
            pos, lat = base[K.POS].double(), base[K.LATTICE][0].double()
            src, dst = g[K.EDGE_INDEX]
            d = (pos[dst] + g[K.EDGE_CELL_SHIFT].double() @ lat - pos[src]).norm(dim=1)
            tei, nti, ntij = threebody_index(int(pos.size(0)), g[K.EDGE_INDEX].numpy(), d.float().numpy(), tb_cutoff)
            g[K.TRIPLET_EDGE_INDEX] = torch.from_numpy(tei)
            g[K.NUM_TRIPLET_I], g[K.NUM_TRIPLET_IJ] = torch.from_numpy(nti), torch.from_numpy(ntij)
            g[K.NUM_EDGES], g[K.NUM_TRIPLETS] = int(g[K.EDGE_INDEX].size(1)), int(tei.shape[1])
            out[(name, vname)] = g
    return out


def dense_cell():
    """(c) the 24-atom cell of test_dense_three_body_rows_beyond_the_staged_window: three-body cutoff 5.0, ~100 partners per centre."""
    return random_cell_graph(24, 5.0, 5, cutoff=5.0, tb_cutoff=5.0, dmin=1.2)


def dense_batch():
    from torch_m3gnet.data.material_graph import Batch

    return Batch.from_data_list([dense_cell()])


# input name -> (builder, the shapes it is run on)
INPUTS = {
    "cells18": (cells18, MFMA_SHAPES + ("any96",)),
    "fcc32": (fcc32, ("default", "any96")),
    "one_sided": (lambda: triplet_list_variants()["one_sided"], ("default",)),
    "thinned": (lambda: triplet_list_variants()["thinned"], ("default",)),
    "asymmetric": (lambda: edge_list_variants()[("thinned", "asymmetric")], ("default",)),
    "dense": (dense_batch, ("dense",)),
}
CONFIGURATIONS = [(shape, name) for name, (_, shapes) in INPUTS.items() for shape in shapes]
LIST_INPUTS = ("one_sided", "thinned", "asymmetric", "dense")   # where angular_t2, tb_basis and dm must each carry 3 %

# ------------------------------------------------------------------ kernel selections (tests/test_gpu_reverse_terms.py runs them)
# name -> (precision, plan options).  Every selection whose reverse pass is an implementation of its own (resolve_step_path,
# csrc/m3g_step_path.h); on these inputs (at most 172 edge tiles, at most 40 atoms) the default is the split-tile pair
# k_edge_block_split / k_edge_rev_split, the moment kernels where the lists are complete, k_node_tb_reverse for blocks > 0.
SELECTIONS = {
    "default": ("fp32", {}),
    "persistent": ("fp32", PERSISTENT),                              # k_edge_block_mfma<SAVE = 2> + k_edge_rev_f32<SAVED_P2>, whole tiles
    "persistent_tail": ("fp32", PERSISTENT_TAIL),                    # ... a workgroup's single tile through rev_split_run
    "persistent_pair": ("fp32", dict(PERSISTENT, rev_kernel=0)),     # node-MLP + edge-MLP kernel pair on saved p1
    "rev_saved_p1": ("fp32", dict(save_p2=0)),                       # k_edge_rev_f32<SAVED_P2 = false>: layer 2 recomputed
    "rev_recompute": ("fp32", dict(save_p1=0, save_p2=0)),           # the pair recomputing both layers
    "pair_saved_p1": ("fp32", dict(rev_kernel=0, save_p2=0)),        # the pair on saved p1, split-tile forward
    "pair_recompute": ("fp32", dict(rev_kernel=0, save_p1=0, save_p2=0)),
    "valu": ("fp32", dict(edge_kernel=0)),                           # vector-ALU baseline kernels
    "any_size": ("fp32", dict(edge_kernel=2)),                       # csrc/m3g_generic.hip
    "list": ("fp32", dict(threebody_moments=0)),                     # three-body list kernels + k_geometry_reverse (moments = 1 is the default)
    "two_launches": ("fp32", dict(fuse_node_tb=0)),                  # three-body reverse and node reverse as launches of their own
    "f16x3": ("f16x3", {}),
    "bf16x3": ("bf16x3", {}),
}
_TBS_ROWS = [(shape, "cells18") for shape in ("tbs1", "tbs2", "tbs3", "tbs4")]
_LISTS = [("default", name) for name in ("one_sided", "thinned", "asymmetric")]
# selection -> the configurations it runs.  All run the default shape on the random cells (where every term carries >= 5 %); the width-96
# shape is beyond every path but the any-size one.
SELECTION_CONFIGS = {sel: [("default", "cells18")] for sel in SELECTIONS}
for _sel in ("default", "persistent", "persistent_pair", "f16x3", "bf16x3"):
    SELECTION_CONFIGS[_sel] += _TBS_ROWS
for _sel in ("default", "persistent", "list", "valu", "any_size", "f16x3", "bf16x3"):
    SELECTION_CONFIGS[_sel] += [("default", "fcc32")]
for _sel in ("default", "persistent", "valu", "any_size"):
    SELECTION_CONFIGS[_sel] += _LISTS
SELECTION_CONFIGS["list"] += [("default", "asymmetric")]   # (its triplet list is complete for the edges that remain: the default takes the moment kernels)
# (the dense cell's windows are beyond the moment kernels' -- its hints word is 0 -- so its default IS the list kernels, long-list
#  instantiation with the global-memory partner path, and threebody_moments = 0 would be the same run again)
for _sel in ("default", "persistent", "valu", "any_size"):
    SELECTION_CONFIGS[_sel] += [("dense", "dense")]
SELECTION_CONFIGS["any_size"] += [("any96", "cells18"), ("any96", "fcc32")]
GPU_CASES = [(sel, shape, name) for sel, configs in SELECTION_CONFIGS.items() for shape, name in configs]


@functools.lru_cache(maxsize=None)
def input_batch(name: str):
    """The host batch of an input (shared: clone before changing it)."""
    return INPUTS[name][0]()


# ------------------------------------------------------------------ oracle evaluations (each formed once, never modified)
def oracle_inputs(model, graph, dtype=torch.float64):
    """(params, cfg, consts, graph dict) of the CPU oracle for a model of the package, constants formed in `dtype`."""
    from test_gpu_properties import _oracle_inputs

    p, cfg, c, og = _oracle_inputs(model, graph)
    p = {k: v.to(dtype) for k, v in p.items()}
    cd = orc.make_constants(cfg, c.elemental_energies, dtype=dtype)
    cd.factors = c.factors.to(dtype)
    return p, cfg, cd, og


@functools.lru_cache(maxsize=None)
def oracle64(shape: str, name: str, weighted=True):
    """fp64 oracle with the exact Legendre derivative on a configuration: what every device result is held against."""
    torch.set_num_threads(8)
    p, cfg, c, og = oracle_inputs(shape_model(shape, name, weighted), input_batch(name))
    return orc.energy_forces(p, cfg, c, og, legendre_backward="exact")


@functools.lru_cache(maxsize=None)
def shares(shape: str, name: str, weighted=True):
    """{term: share of max|F|} of a configuration, from the fp64 staged oracle."""
    torch.set_num_threads(8)
    return staged.term_shares(*oracle_inputs(shape_model(shape, name, weighted), input_batch(name)))
