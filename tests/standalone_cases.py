"""The inputs of the stand-alone module tests, built once and never modified; an fp64 restatement of every module (the oracle's own
stage functions on the upcast fp32 inputs, a few lines of torch where it has none); a second restatement in numpy that carries, beside
each value, the summed moduli of the terms that formed it (`VS`); and the rule that turns the restatement's own fp32 rounding into
the tolerance of the device (`scaled`, `unit`, `MARGIN`).

The rule.  Every output element is measured against its own scale, the summed moduli of its terms (sum |a||b| for a dense product,
carried through sums, products and recurrences by `VS`; an activation keeps the scale of its argument).  The UNIT of a module's output
is the largest scaled deviation of the oracle's restatement evaluated in float32 on the CPU from the same restatement in float64, over
the module's cases.  The device may deviate by MARGIN[...] units.  MARGIN was fixed on the CPU before any GPU run: the numpy restatement
is a second fp32 order (K summed backwards, another libm, other associations of the same products), it needs `second / unit` units,
and MARGIN is twice that, rounded up to an integer (tests/test_standalone_cpu.py::test_margin_covers_a_second_fp32_order holds the
second order to MARGIN / 2 and prints `second / unit` per output).  The units are the rounding of one CPU's fp32 libraries, on one thread
(`all_units`); where another machine's second order needs more than MARGIN / 2 -- `linear` needs 0.9985 of its 1.0 here -- that test fails
and MARGIN is to be recomputed from its printout by the same rule, ceil(2 * second / unit), never from what the device gives.
profiles/standalone_modules.txt lists the units and what the device was measured to need."""
import functools
import math

import numpy as np
import torch

from oracle import m3gnet_oracle as orc

SEED = 7
# units the device may deviate by, per module output: ceil(2 * what the second fp32 order needs), see the module docstring
MARGIN = {
    "linear": 2, "gated_mlp": 2, "edge_weights": 2, "bessel": 3, "edge_distances": 2, "triplet_angles": 3, "mid_edge_features": 2,
    "edge_attr_tb": 2, "x_conv": 2, "edge_attr_conv": 2, "scaled_atomic_energies": 2, "scaled_total_energy": 1, "total_energy": 1,
}


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def t(a, dtype=None):
    """A fresh torch tensor (a copy) of a read-only array."""
    out = torch.tensor(np.array(a))
    return out if dtype is None else out.to(dtype)


# ----------------------------------------------------------------------------------------------------------------- the rule
def scaled(dev, scale):
    """The largest |dev| / scale over the elements with scale > 0; an element of scale 0 (no term at all) must not deviate."""
    dev, scale = np.abs(np.asarray(dev, dtype=np.float64)), np.asarray(scale, dtype=np.float64)
    scale = np.broadcast_to(scale, dev.shape)
    if dev.size == 0:
        return 0.0
    if not np.isfinite(dev).all() or (dev[scale == 0] != 0).any():
        return np.inf
    return float((dev[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


class VS:
    """A value and the summed moduli of the terms that formed it (never below |value|)."""

    def __init__(self, v, s=None):
        self.v = v
        self.s = np.abs(v).astype(np.float64) if s is None else np.maximum(np.asarray(s, dtype=np.float64), np.abs(v))

    def __add__(self, o):
        return VS(self.v + o.v, self.s + o.s)

    def __mul__(self, o):
        return VS(self.v * o.v, self.s * np.abs(o.v) + np.abs(self.v) * o.s)

    def map(self, f):
        return VS(f(self.v), self.s)

    def rows(self, idx):
        return VS(self.v[idx], self.s[idx])


def vs_linear(x: VS, w, b=None, reverse=True):
    """x W^T + b; `reverse`: K walked backwards (a second, equally valid order of the same sum)."""
    w = w.astype(x.v.dtype)
    v = x.v[..., ::-1] @ w[:, ::-1].T if reverse else x.v @ w.T
    s = x.s @ np.abs(w.astype(np.float64)).T
    if b is not None:
        v = v + b.astype(x.v.dtype)
        s = s + np.abs(b.astype(np.float64))
    return VS(v, s)


def np_silu(x):
    return x / (1 + np.exp(-x))


def np_sigmoid(x):
    return 1 / (1 + np.exp(-x))


_ACT = {0: lambda x: x, 1: np_silu, 2: np_sigmoid}


def vs_segment_sum(x: VS, index, n):
    v, s = np.zeros((n,) + x.v.shape[1:], x.v.dtype), np.zeros((n,) + x.v.shape[1:])
    np.add.at(v, index[::-1], x.v[::-1])
    np.add.at(s, index, x.s)
    return VS(v, s)


# ------------------------------------------------------------------------------------------------- special functions, numpy
def np_envelope(d, rc3):
    rho = d / d.dtype.type(rc3)
    inside = rho <= 1
    v = 1 - 6 * rho**5 + 15 * rho**4 - 10 * rho**3
    s = 1 + 6 * rho**5 + 15 * rho**4 + 10 * rho**3
    return VS(np.where(inside, v, 0).astype(d.dtype), np.where(inside, s, 0))


def np_legendre(x, L):
    """[P_0 .. P_{L-1}] by Bonnet's recursion."""
    one = np.ones_like(x)
    p = [VS(one), VS(x)]
    for n in range(1, L - 1):
        v = ((2 * n + 1) * x * p[n].v - n * p[n - 1].v) / (n + 1)
        s = ((2 * n + 1) * np.abs(x) * p[n].s + n * p[n - 1].s) / (n + 1)
        p.append(VS(v.astype(x.dtype), s))
    return p[:L]


def np_sph_bessel(x, L):
    """[j_0 .. j_{L-1}] by the upward recurrence with the x <= 1e-8 branch.  The argument carries its own rounding, which moves sin and
    cos by that rounding times the argument: the scales start from |sin| + |cos|, not from |sin| alone."""
    big = x > 1e-8
    xs = np.where(big, x, 1).astype(x.dtype)
    sn, cs = np.sin(xs), np.cos(xs)
    base = (np.abs(sn) + np.abs(cs)).astype(np.float64)
    v, s = [sn / xs, (sn / xs - cs) / xs], [base / np.minimum(xs, 1), (base / np.minimum(xs, 1) + base) / xs]
    for n in range(1, L - 1):
        v.append(((2 * n + 1) / xs * v[n] - v[n - 1]).astype(x.dtype))
        s.append((2 * n + 1) / xs * s[n] + s[n - 1])
    out, dfact = [], 1.0
    for l in range(L):
        if l > 0:
            dfact *= 2 * l + 1
        small = np.ones_like(x) if l == 0 else (x / x.dtype.type(dfact))
        out.append(VS(np.where(big, v[l], small).astype(x.dtype), np.where(big, s[l], np.abs(small))))
    return out


# ------------------------------------------------------------------------------------------------------------ constants
def radial_constants(n_max, cutoff):
    cfg = orc.OracleConfig(cutoff=cutoff, n_max=n_max, l_max=1)
    c = orc.make_constants(cfg)
    return cfg, c


def basis_constants(l_max, n_max, cutoff, threebody_cutoff=None):
    """(cfg, constants) with the documented normalisation, as the tests of the three-body path use it."""
    cfg = orc.OracleConfig(cutoff=cutoff, threebody_cutoff=cutoff if threebody_cutoff is None else threebody_cutoff, l_max=l_max, n_max=n_max)
    c = orc.make_constants(cfg)
    c.factors = orc.documented_factors(cfg)
    return cfg, c


def _cast(c: orc.OracleConstants, dtype):
    return orc.OracleConstants(c.em.to(dtype), c.dm.to(dtype), c.coeff.to(dtype), c.factors.to(dtype), c.zeros.to(dtype),
                               None if c.elemental_energies is None else c.elemental_energies.to(dtype))


# ---------------------------------------------------------------------------------------- restatements: torch (the oracle's)
def ref_linear(x, w, b, act, dtype):
    y = torch.nn.functional.linear(t(x, dtype), t(w, dtype), None if b is None else t(b, dtype))
    return (y, torch.nn.functional.silu(y), torch.sigmoid(y))[act].numpy()


def ref_gated_mlp(x, params, n_layers, is_output, use_bias, dtype):
    p = {f"m.{k}": t(v, dtype) for k, v in params.items()}
    return orc.gated_mlp(t(x, dtype), p, "m", n_layers, is_output=is_output, use_bias=use_bias).numpy()


def ref_edge_weights(dist, cfg, c, dtype):
    return orc.radial_basis(t(dist, dtype), cfg, _cast(c, dtype)).numpy()


def ref_bessel(rs, cfg, c, dtype):
    return orc.normalized_sbf(t(rs, dtype), cfg, _cast(c, dtype)).numpy()


def ref_distance_angle(g, length_scale, dtype):
    pos, lat = t(g["pos"], dtype) / length_scale, t(g["lattice"], dtype) / length_scale
    d, a = orc.distance_and_angle(pos, lat, t(g["batch"]).long(), t(g["edge_index"]).long(), t(g["edge_cell_shift"]), t(g["triplet_edge_index"]).long())
    return d.numpy(), a.numpy()


def ref_three_body(case, dtype, order=None):
    """(mid [E,C], edge_attr [E,D]) of ThreeBodyInteration.forward; `order`: a permutation of the triplets."""
    g, cfg, c = case["graph"], case["cfg"], _cast(case["consts"], dtype)
    p = {f"m.{k}": t(v, dtype) for k, v in case["params"].items()}
    tei, ang = t(g["triplet_edge_index"]).long(), t(case["angles"], dtype)
    if order is not None:
        tei, ang = tei[:, order], ang[order]
    mid = orc.three_body_mid(t(case["x"], dtype), t(case["dist"], dtype), ang, t(g["edge_index"]).long(), tei, p, "m", cfg, c, "exact")
    e = t(case["e"], dtype) + orc.gated_mlp(mid, p, "m.gated_mlp", 1, use_bias=False)
    return mid.numpy(), e.numpy()


def ref_conv(case, dtype):
    p = {f"m.{k}": t(v, dtype) for k, v in case["params"].items()}
    x, e = orc.conv_block(t(case["x"], dtype), t(case["e"], dtype), t(case["h"], dtype), t(case["graph"]["edge_index"]).long(), p, "m")
    return x.numpy(), e.numpy()


def ref_readout(case, dtype, order=None):
    """(scaled_atomic [N], scaled_total [S], total [S]) of AtomWiseReadout.forward (nn/readout.py:39-58); `order`: the order in which
    the atoms are added to their structures' sums."""
    p = {f"m.{k}": t(v, dtype) for k, v in case["params"].items()}
    atomic = orc.gated_mlp(t(case["x"], dtype), p, "m.gated", 3, is_output=True)[:, 0]
    ea = t(case["elemental"], dtype) / case["energy_scale"] + atomic
    batch = t(case["batch"]).long()
    if order is None:
        st = torch.zeros(case["S"], dtype=dtype).index_add(0, batch, ea)
    else:   # the atoms added one by one in the given order
        st = torch.zeros(case["S"], dtype=dtype)
        for a in order:
            st[batch[a]] += ea[a]
    return ea.numpy(), st.numpy(), (case["energy_scale"] * st).numpy()


# ------------------------------------------------------------------- restatements: numpy, with scales (the second fp32 order)
def np_linear(x, w, b, act, dtype):
    y = vs_linear(VS(np.asarray(x, dtype)), np.asarray(w), None if b is None else np.asarray(b))
    return y.map(_ACT[act])


def np_gated_mlp(x: VS, params, prefix, n_layers, is_output=False, use_bias=True):
    d = g = x
    for i in range(n_layers):
        last = i == n_layers - 1
        bd = np.asarray(params[f"{prefix}dense.{2 * i}.bias"]) if use_bias else None
        bg = np.asarray(params[f"{prefix}gate.{2 * i}.bias"]) if use_bias else None
        d = vs_linear(d, np.asarray(params[f"{prefix}dense.{2 * i}.weight"]), bd)
        g = vs_linear(g, np.asarray(params[f"{prefix}gate.{2 * i}.weight"]), bg)
        if not (is_output and last):
            d = d.map(np_silu)
        g = g.map(np_sigmoid if last else np_silu)
    return d * g


def np_edge_weights(dist, cfg, c, dtype):
    """The sinc arguments are as large as pi (n_max + 1) pi and carry their own rounding, which moves sinc by at most that rounding:
    each sinc counts with the modulus 1."""
    d = np.asarray(dist, dtype)
    em, dm, coeff = (np.asarray(a.numpy(), dtype) for a in (c.em, c.dm, c.coeff))
    h, out = None, []
    for m in range(cfg.n_max):
        # (m + 1) pi / rc is formed in float32 whatever the type of the distances, as the reference forms it: a constant of the module
        a1, a2 = (dtype(np.float32(k) * np.float32(np.pi) / np.float32(cfg.scaled_cutoff)) for k in (m + 1, m + 2))
        f = VS((coeff[m] * (np.sinc(a1 * d) + np.sinc(a2 * d))).astype(dtype), 2 * abs(float(coeff[m])) * np.ones(d.shape))
        if m > 0:
            mul, div = np.sqrt(em[m] / dm[m - 1]), np.sqrt(dm[m])
            f = VS(((f.v + mul * h.v) / div).astype(dtype), (f.s + float(mul) * h.s) / float(div))
        h = f
        out.append(f)
    return VS(np.stack([o.v for o in out], 1), np.stack([o.s for o in out], 1))


def np_chi(r, cfg, c, dtype):
    """[l_max, n_max, len(r)]"""
    z, f = np.asarray(c.zeros.numpy(), dtype), np.asarray(c.factors.numpy(), dtype)
    r = np.asarray(r, dtype)
    v, s = [], []
    for l in range(cfg.l_max):
        x = (z[l][: cfg.n_max, None] * r[None, :] / dtype(cfg.scaled_cutoff)).astype(dtype)
        j = np_sph_bessel(x, l + 1)[l]
        v.append((j.v / f[l][:, None]).astype(dtype))
        s.append(j.s / np.abs(f[l][:, None].astype(np.float64)))
    return VS(np.stack(v), np.stack(s))


def np_distance_angle(g, length_scale, dtype):
    pos, lat = np.asarray(g["pos"], dtype) / dtype(length_scale), np.asarray(g["lattice"], dtype) / dtype(length_scale)
    ei, tei, sh = np.asarray(g["edge_index"]), np.asarray(g["triplet_edge_index"]), np.asarray(g["edge_cell_shift"]).astype(dtype)
    le = lat[np.asarray(g["batch"])[ei[0]]]                       # [E,3,3]
    sv = VS(sh[:, 2, None] * le[:, 2]) + VS(sh[:, 1, None] * le[:, 1]) + VS(sh[:, 0, None] * le[:, 0])
    vec = VS(-pos[ei[0]]) + (sv + VS(pos[ei[1]]))
    d = np.sqrt((vec.v**2).sum(1)).astype(dtype)
    ds = np.sqrt((vec.s**2).sum(1))                               # |dd| <= |dvec|
    u = vec.v / d[:, None]
    cos = np.clip((u[tei[0]] * u[tei[1]]).sum(1), -1, 1).astype(dtype)
    rel = (vec.s / np.maximum(d[:, None].astype(np.float64), 1e-300)).sum(1)
    return VS(d, ds), VS(cos, 1 + rel[tei[0]] + rel[tei[1]])


def np_three_body(case, dtype):
    g, cfg, c = case["graph"], case["cfg"], case["consts"]
    ei, tei = np.asarray(g["edge_index"]), np.asarray(g["triplet_edge_index"])
    p = case["params"]
    dist, ang = np.asarray(case["dist"], dtype), np.asarray(case["angles"], dtype)
    E, C = dist.shape[0], cfg.l_max * cfg.n_max
    fc = np_envelope(dist, cfg.scaled_threebody_cutoff)
    v = vs_linear(VS(np.asarray(case["x"], dtype)), np.asarray(p["linear_sigmoid1.weight"]), np.asarray(p["linear_sigmoid1.bias"])).map(np_sigmoid)
    P = np_legendre(ang, cfg.l_max)
    chi = np_chi(dist[tei[1]], cfg, c, dtype)                     # [L,R,T]
    k = ei[1][tei[1]]
    f2 = fc.rows(tei[0]) * fc.rows(tei[1])
    cols = []
    for l in range(cfg.l_max):
        y = VS((dtype(math.sqrt((2 * l + 1) / (4 * math.pi))) * P[l].v).astype(dtype), math.sqrt((2 * l + 1) / (4 * math.pi)) * P[l].s) * f2
        for n in range(cfg.n_max):
            term = VS(chi.v[l, n], chi.s[l, n]) * y * VS(v.v[k, l * cfg.n_max + n], v.s[k, l * cfg.n_max + n])
            cols.append(vs_segment_sum(term, tei[0], E))
    mid = VS(np.stack([c_.v for c_ in cols], 1).reshape(E, C), np.stack([c_.s for c_ in cols], 1).reshape(E, C))
    upd = np_gated_mlp(mid, p, "gated_mlp.", 1, use_bias=False)
    return mid, VS(np.asarray(case["e"], dtype)) + upd


def np_conv(case, dtype):
    ei, p = np.asarray(case["graph"]["edge_index"]), case["params"]
    x, e, h = (VS(np.asarray(case[k], dtype)) for k in ("x", "e", "h"))

    def cat(e_):
        return VS(np.concatenate([x.v[ei[0]], x.v[ei[1]], e_.v], 1), np.concatenate([x.s[ei[0]], x.s[ei[1]], e_.s], 1))

    e = e + np_gated_mlp(cat(e), p, "concat_edge_update.", 2) * vs_linear(h, np.asarray(p["edge_linear.weight"]))
    msg = np_gated_mlp(cat(e), p, "concat_node_update.", 2) * vs_linear(h, np.asarray(p["node_linear.weight"]))
    return x + vs_segment_sum(msg, ei[0], x.v.shape[0]), e


def np_readout(case, dtype):
    a = np_gated_mlp(VS(np.asarray(case["x"], dtype)), case["params"], "gated.", 3, is_output=True)
    ea = VS(np.asarray(case["elemental"], dtype) / dtype(case["energy_scale"])) + VS(a.v[:, 0], a.s[:, 0])
    st = vs_segment_sum(ea, np.asarray(case["batch"]), case["S"])
    return ea, st, VS((dtype(case["energy_scale"]) * st.v).astype(dtype), abs(case["energy_scale"]) * st.s)


# ------------------------------------------------------------------------------------------------------------------ inputs
LINEAR_ROWS, LINEAR_IN, LINEAR_OUT = (0, 1, 63, 64, 65, 130), (1, 15, 16, 17, 192), (1, 15, 16, 17, 64, 65)


@functools.lru_cache(maxsize=None)
def linear_case(n, k, out):
    """(x [n,k], w [out,k], b [out]) -- rows 63 / 64 / 65 / 130 sit below, on, above one 64-row tile of g_gemm and in its third tile;
    k = 15 / 16 / 17 around one 16-deep slab, 192 twelve slabs; out = 15 / 16 / 17 around one 16-column block, 64 / 65 around the
    64-column tile."""
    rng = np.random.default_rng([SEED, n, k, out])
    return _ro(rng.normal(0, 1, (n, k)).astype(np.float32)), _ro(rng.normal(0, 1 / math.sqrt(k), (out, k)).astype(np.float32)), \
        _ro(rng.normal(0, 0.5, out).astype(np.float32))


def _mlp_params(rng, prefix, widths, use_bias=True):
    p = {}
    for i in range(len(widths) - 1):
        for br in ("dense", "gate"):
            p[f"{prefix}{br}.{2 * i}.weight"] = _ro(rng.normal(0, 1.5 / math.sqrt(widths[i]), (widths[i + 1], widths[i])).astype(np.float32))
            if use_bias:
                p[f"{prefix}{br}.{2 * i}.bias"] = _ro(rng.normal(0, 0.3, widths[i + 1]).astype(np.float32))
    return p


@functools.lru_cache(maxsize=None)
def index_graph(n_atoms, hub_edges, n_structs=1):
    """Index tensors only (no geometry): atom 0 is the centre of `hub_edges` edges, every other atom of two; edges sorted by centre.
    Triplets: every ordered pair of the two edges of a plain atom; at the hub the FIRST edge paired with every other one, both ways
    (so edge 0 is e1 of hub_edges - 1 triplets: contended atomics of the stand-alone aggregate).  batch: structure s holds the atoms
    a with a % n_structs == s -- unsorted on purpose -- except the LAST structure, which holds none when n_structs > 1."""
    src, dst = [], []
    if n_atoms > 1:
        for k in range(hub_edges):
            src.append(0), dst.append(1 + k % (n_atoms - 1))
        for a in range(1, n_atoms):
            for step in (1, 2):
                src.append(a), dst.append((a + step) % n_atoms)
    ei = np.array([src, dst], dtype=np.int64).reshape(2, -1)
    t0, t1 = [], []
    for k in range(1, hub_edges if n_atoms > 1 else 0):
        t0 += [0, k]
        t1 += [k, 0]
    for a in range(1, n_atoms):
        e0 = hub_edges + 2 * (a - 1)
        t0 += [e0, e0 + 1]
        t1 += [e0 + 1, e0]
    tei = np.array([t0, t1], dtype=np.int64).reshape(2, -1)
    filled = max(n_structs - 1, 1)
    batch = np.arange(n_atoms, dtype=np.int64) % filled
    return dict(edge_index=_ro(ei), triplet_edge_index=_ro(tei), batch=_ro(batch),
                lattice=_ro(np.tile(np.eye(3, dtype=np.float32) * 9, (n_structs, 1, 1))))


def drop_edges(g):
    """The same atoms without edges (E = 0, T = 0)."""
    return dict(g, edge_index=_ro(np.zeros((2, 0), np.int64)), triplet_edge_index=_ro(np.zeros((2, 0), np.int64)))


THREE_BODY_SHAPES = [(1, 1, 1), (3, 3, 64), (4, 4, 64), (9, 10, 24), (5, 4, 96)]


@functools.lru_cache(maxsize=None)
def three_body_case(l_max, n_max, D, kind="hub"):
    """kind: "hub" (20 atoms, one edge with 300 triplets), "T0" (edges, no triplet), "E0" (atoms only)."""
    rng = np.random.default_rng([SEED, 3, l_max, n_max, D])
    g = index_graph(20, 301)
    if kind == "T0":
        g = dict(g, triplet_edge_index=_ro(np.zeros((2, 0), np.int64)))
    if kind == "E0":
        g = drop_edges(g)
    cfg, c = basis_constants(l_max, n_max, 5.0, 4.0)
    E, T, C = g["edge_index"].shape[1], g["triplet_edge_index"].shape[1], l_max * n_max
    dist = rng.uniform(0.7, 4.3, E).astype(np.float32)           # some beyond the three-body cutoff: their envelope is 0
    if E:
        dist[0] = 2.0
    params = {"linear_sigmoid1.weight": _ro(rng.normal(0, 1 / math.sqrt(D), (C, D)).astype(np.float32)),
              "linear_sigmoid1.bias": _ro(rng.normal(0, 0.3, C).astype(np.float32))}
    params.update(_mlp_params(rng, "gated_mlp.", [C, D], use_bias=False))
    return dict(graph=g, cfg=cfg, consts=c, params=params, dist=_ro(dist), angles=_ro(rng.uniform(-1, 1, T).astype(np.float32)),
                x=_ro(rng.normal(0, 1, (20, D)).astype(np.float32)), e=_ro(rng.normal(0, 1, (E, D)).astype(np.float32)), l_max=l_max, n_max=n_max, D=D)


CONV_SHAPES = [(1, 1), (24, 3), (64, 10), (96, 3), (64, 1), (24, 10)]   # every D of {1, 24, 64, 96} and every R of {1, 3, 10}


@functools.lru_cache(maxsize=None)
def conv_case(D, R, kind="hub"):
    """kind: "hub": 65 atoms, atom 0 the centre of 70 edges; "E0": the same atoms without edges."""
    rng = np.random.default_rng([SEED, 4, D, R])
    g = index_graph(65, 70)
    if kind == "E0":
        g = drop_edges(g)
    E = g["edge_index"].shape[1]
    params = {}
    for name, last in (("concat_edge_update.", D), ("concat_node_update.", D)):
        params.update(_mlp_params(rng, name, [3 * D, D, last]))
    params["edge_linear.weight"] = _ro(rng.normal(0, 1 / math.sqrt(R), (D, R)).astype(np.float32))
    params["node_linear.weight"] = _ro(rng.normal(0, 1 / math.sqrt(R), (D, R)).astype(np.float32))
    return dict(graph=g, params=params, x=_ro(rng.normal(0, 1, (65, D)).astype(np.float32)), e=_ro(rng.normal(0, 1, (E, D)).astype(np.float32)),
                h=_ro(rng.normal(0, 1, (E, R)).astype(np.float32)), D=D, R=R)


READOUT_SHAPES = [(D, N, S, scale) for D, N, S in ((1, 1, 1), (64, 65, 4), (96, 65, 1), (64, 0, 4), (1, 65, 4), (96, 1, 4), (64, 0, 1))
                  for scale in ((1e-6, 1.0, 1e6) if (D, N, S) == (64, 65, 4) else (1.0,))]


@functools.lru_cache(maxsize=None)
def readout_case(D, N, S, energy_scale):
    rng = np.random.default_rng([SEED, 5, D, N, S])
    g = index_graph(N, 3, S) if N else dict(edge_index=_ro(np.zeros((2, 0), np.int64)), triplet_edge_index=_ro(np.zeros((2, 0), np.int64)),
                                            batch=_ro(np.zeros(0, np.int64)), lattice=_ro(np.tile(np.eye(3, dtype=np.float32) * 9, (S, 1, 1))))
    batch = np.array(g["batch"])
    if N > 3:
        batch = batch[rng.permutation(N)]                          # unsorted
    return dict(graph=g, params=_mlp_params(rng, "gated.", [D, D, D, 1]), x=_ro(rng.normal(0, 1, (N, D)).astype(np.float32)),
                elemental=_ro(rng.normal(0, 3, N).astype(np.float32)), batch=_ro(batch), S=S, energy_scale=energy_scale, D=D, N=N)


EDGE_CUTOFF = 5.0


@functools.lru_cache(maxsize=None)
def edge_distances(n_edges):
    """0, 1e-4, the cutoff, its two float32 neighbours and beyond it first; then uniform over [0.3, 1.2 cutoff]."""
    rc = np.float32(EDGE_CUTOFF)
    edge = [0.0, 1e-4, rc, np.nextafter(rc, np.float32(0)), np.nextafter(rc, np.float32(10)), 1.3 * EDGE_CUTOFF]
    d = np.concatenate([edge, np.random.default_rng([SEED, 6]).uniform(0.3, 1.2 * EDGE_CUTOFF, max(n_edges - len(edge), 0))])[:n_edges]
    return _ro(d.astype(np.float32))


BESSEL_CORNERS = [(l, n) for l in (1, 9) for n in (1, 10)]
BESSEL_CUTOFF = 4.2


@functools.lru_cache(maxsize=None)
def bessel_radii(n):
    """r >= 0.6 A (below it the upward recurrence is held to the reference's own noise by the existing small-r tests), the cutoff
    included."""
    r = np.linspace(0.6, BESSEL_CUTOFF, n) if n > 1 else np.array([2.0])
    return _ro(r[:n].astype(np.float32))


@functools.lru_cache(maxsize=None)
def geometry_graphs():
    """The graphs of the DistanceAndAngle tests: the triclinic left-handed `tri` fixture, a batch of two random cells, a cell whose
    atoms are out of each other's reach (E = 0), and a cell with edges but no triplet (T = 0: three-body cutoff below every distance)."""
    from torch_m3gnet.data.material_graph import Batch, MaterialGraph
    from torch_m3gnet.data.synthetic import random_cell_arrays, random_cell_graph

    keys = ("pos", "lattice", "batch", "edge_index", "edge_cell_shift", "triplet_edge_index", "atom_types")
    tri, _ = orc.load_case_npz(_golden() / "case_tri_ref.npz")
    out = {"tri": tri,
           "pair": Batch.from_data_list([random_cell_graph(9, 5.2, 1, cutoff=3.6, tb_cutoff=3.0), random_cell_graph(7, 4.9, 2, cutoff=3.6, tb_cutoff=3.0)]),
           "E0": Batch.from_data_list([MaterialGraph.from_arrays(np.eye(3) * 12.0, np.array([[0, 0, 0], [6.0, 6, 6], [0, 6, 0]]), [3, 5, 7], 3.0, 3.0)]),
           "T0": Batch.from_data_list([MaterialGraph.from_arrays(*random_cell_arrays(6, 4.8, 3, dmin=2.0), 3.6, 1.0)])}
    return {name: {k: _ro(g[k].numpy()) for k in keys} for name, g in out.items()}


def _golden():
    from pathlib import Path

    return Path(__file__).resolve().parent / "golden"


# ------------------------------------------------------------------------------------------------------- units, per module
def _worst(pairs):
    return max([scaled(a - b, s) for a, b, s in pairs] + [0.0])


@functools.lru_cache(maxsize=None)
def linear_units():
    """(unit, what the second fp32 order needs) of m3g_linear over the whole shape grid, every activation, with bias."""
    first, second = [], []
    for act in (0, 1, 2):
        for n in LINEAR_ROWS:
            for k in LINEAR_IN:
                for o in LINEAR_OUT:
                    x, w, b = linear_case(n, k, o)
                    hi, y2 = ref_linear(x, w, b, act, torch.float64), np_linear(x, w, b, act, np.float32)
                    scale = np_linear(x, w, b, act, np.float64).s
                    first.append((ref_linear(x, w, b, act, torch.float32), hi, scale))
                    second.append((y2.v, hi, scale))
    return _worst(first), _worst(second)


def linear_scale(x, w, b, act=0):
    return np_linear(x, w, b, act, np.float64).s


@functools.lru_cache(maxsize=None)
def edge_weight_units():
    first, second = [], []
    for degree in range(1, 11):
        cfg, c = radial_constants(degree, EDGE_CUTOFF)
        d = edge_distances(257)
        hi, s = ref_edge_weights(d, cfg, c, torch.float64), np_edge_weights(d, cfg, c, np.float64).s
        first.append((ref_edge_weights(d, cfg, c, torch.float32), hi, s))
        second.append((np_edge_weights(d, cfg, c, np.float32).v, hi, s))
    return _worst(first), _worst(second)


@functools.lru_cache(maxsize=None)
def bessel_units():
    first, second = [], []
    for l, n in BESSEL_CORNERS:
        cfg, c = basis_constants(l, n, BESSEL_CUTOFF)
        r = bessel_radii(257)
        hi, s = ref_bessel(r, cfg, c, torch.float64), np_chi(r, cfg, c, np.float64).s
        first.append((ref_bessel(r, cfg, c, torch.float32), hi, s))
        second.append((np_chi(r, cfg, c, np.float32).v, hi, s))
    return _worst(first), _worst(second)


GEOMETRY_SCALES = (1.0, 1.7)


@functools.lru_cache(maxsize=None)
def geometry_units():
    """{"edge_distances": (unit, second), "triplet_angles": (unit, second)}"""
    first, second = {"edge_distances": [], "triplet_angles": []}, {"edge_distances": [], "triplet_angles": []}
    for g in geometry_graphs().values():
        for ls in GEOMETRY_SCALES:
            hi, lo = ref_distance_angle(g, ls, torch.float64), ref_distance_angle(g, ls, torch.float32)
            sc, v2 = np_distance_angle(g, ls, np.float64), np_distance_angle(g, ls, np.float32)
            for i, name in enumerate(first):
                first[name].append((lo[i], hi[i], sc[i].s))
                second[name].append((v2[i].v, hi[i], sc[i].s))
    return {name: (_worst(first[name]), _worst(second[name])) for name in first}


@functools.lru_cache(maxsize=None)
def three_body_units():
    """The aggregate is formed with float atomics on the device, in an order that varies from run to run: the unit is taken over 8
    random triplet orders of the fp32 restatement."""
    first, second = {"mid_edge_features": [], "edge_attr_tb": []}, {"mid_edge_features": [], "edge_attr_tb": []}
    rng = np.random.default_rng([SEED, 8])
    for shape in THREE_BODY_SHAPES:
        case = three_body_case(*shape)
        hi, sc, v2 = ref_three_body(case, torch.float64), np_three_body(case, np.float64), np_three_body(case, np.float32)
        T = case["angles"].shape[0]
        for _ in range(8):
            lo = ref_three_body(case, torch.float32, order=torch.tensor(rng.permutation(T)))
            for i, name in enumerate(first):
                first[name].append((lo[i], hi[i], sc[i].s))
        for i, name in enumerate(first):
            second[name].append((v2[i].v, hi[i], sc[i].s))
    return {name: (_worst(first[name]), _worst(second[name])) for name in first}


@functools.lru_cache(maxsize=None)
def conv_units():
    first, second = {"x_conv": [], "edge_attr_conv": []}, {"x_conv": [], "edge_attr_conv": []}
    for shape in CONV_SHAPES:
        case = conv_case(*shape)
        hi, lo, sc, v2 = ref_conv(case, torch.float64), ref_conv(case, torch.float32), np_conv(case, np.float64), np_conv(case, np.float32)
        for i, name in enumerate(first):
            first[name].append((lo[i], hi[i], sc[i].s))
            second[name].append((v2[i].v, hi[i], sc[i].s))
    return {name: (_worst(first[name]), _worst(second[name])) for name in first}


READOUT_OUTPUTS = ("scaled_atomic_energies", "scaled_total_energy", "total_energy")


@functools.lru_cache(maxsize=None)
def readout_units():
    """The structures' sums are formed with float atomics on the device, like the three-body aggregate: their units are taken over 8
    random atom orders of the fp32 restatement as well."""
    first, second = {k: [] for k in READOUT_OUTPUTS}, {k: [] for k in READOUT_OUTPUTS}
    rng = np.random.default_rng([SEED, 10])
    for shape in READOUT_SHAPES:
        case = readout_case(*shape)
        hi, sc, v2 = ref_readout(case, torch.float64), np_readout(case, np.float64), np_readout(case, np.float32)
        for rep in range(8):
            lo = ref_readout(case, torch.float32, order=None if rep == 0 else rng.permutation(case["N"]))
            for i, name in enumerate(READOUT_OUTPUTS):
                first[name].append((lo[i], hi[i], sc[i].s))
        for i, name in enumerate(READOUT_OUTPUTS):
            second[name].append((v2[i].v, hi[i], sc[i].s))
    return {name: (_worst(first[name]), _worst(second[name])) for name in first}


GATED_MLP_SHAPES = [(9, (64,), False, False), (192, (64, 64), False, True), (17, (33, 5, 1), True, True)]


@functools.lru_cache(maxsize=None)
def gated_mlp_case(in_features, dims, is_output, use_bias, rows=130):
    rng = np.random.default_rng([SEED, 9, in_features, len(dims)])
    return dict(params=_mlp_params(rng, "", [in_features, *dims], use_bias), x=_ro(rng.normal(0, 1, (rows, in_features)).astype(np.float32)),
                dims=dims, is_output=is_output, use_bias=use_bias)


@functools.lru_cache(maxsize=None)
def gated_mlp_units():
    first, second = [], []
    for shape in GATED_MLP_SHAPES:
        c = gated_mlp_case(*shape)
        args = (c["params"], len(c["dims"]), c["is_output"], c["use_bias"])
        hi = ref_gated_mlp(c["x"], *args, torch.float64)
        sc = np_gated_mlp(VS(np.asarray(c["x"], np.float64)), c["params"], "", len(c["dims"]), c["is_output"], c["use_bias"]).s
        first.append((ref_gated_mlp(c["x"], *args, torch.float32), hi, sc))
        second.append((np_gated_mlp(VS(np.asarray(c["x"], np.float32)), c["params"], "", len(c["dims"]), c["is_output"], c["use_bias"]).v, hi, sc))
    return _worst(first), _worst(second)


@functools.lru_cache(maxsize=None)
def all_units():
    """{output name: (unit, what the second fp32 order needs)} for every key of MARGIN.  Evaluated on ONE thread: the unit is the rounding
    of torch's fp32 products, whose summation order follows the number of threads, and MARGIN was fixed against the one-thread figures."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = {"linear": linear_units(), "gated_mlp": gated_mlp_units(), "edge_weights": edge_weight_units(), "bessel": bessel_units()}
        for d in (geometry_units(), three_body_units(), conv_units(), readout_units()):
            out.update(d)
    finally:
        torch.set_num_threads(threads)
    return out


def unit(name):
    u = all_units()[name][0]
    assert 0.0 < u < np.inf, (name, u)
    return u


def bound(name):
    """What the device's scaled deviation of `name` must stay within."""
    return MARGIN[name] * unit(name)
