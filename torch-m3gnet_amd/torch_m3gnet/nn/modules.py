"""`torch_m3gnet.nn` modules: same class names, constructor signatures, attribute names and
`state_dict` keys as the reference -- the compute is libm3gnet_hip.so.

Every module keeps the reference protocol `forward(graph) -> graph` (mutates and returns the keyed
container).  `Gradient(Sequential(...))` as assembled by `build_model` runs the whole path as ONE
fused engine call (m3g_energy_forces).  The cheap leading modules (ScaleLength, AtomRef,
DistanceAndAngle, AtomFeaturizer, EdgeFeaturizer) can also run on their own through the C-ABI
stage entry points, as the reference's unit tests use them, and so can the block modules (EdgeAdjustor,
GatedMLP, NormalizedSphericalBessel, ThreeBodyInteration, M3GNetConv, AtomWiseReadout: m3g_linear, m3g_three_body,
m3g_conv_block, m3g_readout -- run-time-sized fp32 kernels, forward only): the bare `Sequential` is callable like
the reference's (tests/test_model.py:14-38).

Parameter creation order follows the reference so that a given `torch.manual_seed` yields the same
initial weights; constants (`em`, `dm`, `coeff`, `factors`) are built with the same fp32 torch
arithmetic because the reference treats them as captured, platform-dependent values
(SURVEY finding 1).  Outputs are plain tensors: this is an inference engine, nothing is attached
to an autograd graph.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .. import _cuda, _lib
from ..data import MaterialGraphKey as K
from ._bessel_zeros import SPHERICAL_BESSEL_ZEROS


# ----------------------------------------------------------------------------------------------
# host-side special functions (constant set-up and API parity only; never on the per-step path)
def spherical_bessel(x: torch.Tensor, order: int) -> torch.Tensor:
    """j_order(x): upward recurrence with the small-argument branch (reference nn/interaction.py:284-318)."""
    if order < 0:
        raise AssertionError("order must be non-negative")
    tiny = 1e-8
    safe = x > tiny
    ratio = torch.sin(x) / x
    cur = torch.where(safe, ratio, torch.ones_like(x))
    if order == 0:
        return cur
    prev, cur = cur, torch.where(safe, (ratio - torch.cos(x)) / x, x / 3)
    denom = 3
    for n in range(1, order):
        denom *= 2 * n + 3
        prev, cur = cur, torch.where(safe, (2 * n + 1) / x * cur - prev, x / denom)
    return cur


def legendre_cos(x: torch.Tensor, order: int) -> torch.Tensor:
    """Legendre polynomial P_order(x) (reference nn/interaction.py:353-365); plain autograd, exact derivative."""
    if order < 0:
        raise AssertionError("order must be non-negative")
    prev, cur = torch.ones_like(x), x
    if order == 0:
        return prev
    for n in range(1, order):
        prev, cur = cur, ((2 * n + 1) * x * cur - n * prev) / (n + 1)
    return cur


def cutoff_function(r: torch.Tensor, cutoff: float) -> torch.Tensor:
    """Polynomial envelope 1 - 6 t^5 + 15 t^4 - 10 t^3, t = r / cutoff, zero beyond (nn/interaction.py:389-400)."""
    t = r / cutoff
    return torch.where(t <= 1, 1 - 6 * t**5 + 15 * t**4 - 10 * t**3, torch.zeros_like(r))


# ----------------------------------------------------------------------------------------------
def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(
            f"torch_m3gnet (MI355X build): '{what}' must be a GPU tensor -- this package has no CPU path "
            "(move the graph with graph.to('cuda'))"
        )


def _ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


_stream = _cuda.stream_ptr


class _Topology:
    """Device-side CSR form of a graph's index tensors (m3g_topology_build), cached on the graph."""

    # form the three-body certificate (m3g_topology_hints) together with the build: one wait for the device instead of two.  False:
    # build only; `query_hints` then asks for the certificate on demand
    WITH_HINTS = True

    def __init__(self, graph, sig=None) -> None:
        """`sig`: `signature(graph)` when the caller has just formed it."""
        lib = _lib.load_library()
        ei, tei, batch = graph[K.EDGE_INDEX], graph[K.TRIPLET_EDGE_INDEX], graph[K.BATCH]
        for t, name in ((ei, K.EDGE_INDEX), (tei, K.TRIPLET_EDGE_INDEX), (batch, K.BATCH)):
            _require_cuda(t, name)
        self.ei = ei.contiguous().long()
        self.tei = tei.contiguous().long()
        self.batch = batch.contiguous().long()
        self.N, self.E, self.T = int(self.batch.numel()), int(self.ei.size(1)), int(self.tei.size(1))
        self.S = int(graph[K.LATTICE].size(0))
        nbytes = C.c_size_t()
        _lib.check(lib.m3g_topology_bytes(self.N, self.E, self.T, self.S, C.byref(nbytes)))
        self.buf = torch.empty(nbytes.value, dtype=torch.uint8, device=self.ei.device)
        self._pending = None
        # lists written by this library's own builders and untouched since (graph_gpu.mark_canonical): the build skips the checks
        # those lists pass by construction
        is_dict = isinstance(graph, dict)
        canonical = is_dict and graph.get("_m3g_canonical_lists") == (sig if sig is not None else self.signature(graph))
        # a trajectory graph (data/md.py) brings pinned host memory for the build's verdict: the build is then only QUEUED here and
        # `finish` -- called by whoever needs the buffer -- waits for it, so the host prepares the engine call meanwhile
        verdict = graph.get("_m3g_pinned_verdict") if is_dict else None
        with _cuda.on_device(self.buf.device):
            if canonical and verdict is not None and self.WITH_HINTS:
                stream = _stream()
                _lib.check(lib.m3g_topology_build_canonical_begin(self.N, self.E, self.T, self.S, _ptr(self.ei), _ptr(self.tei), _ptr(self.batch),
                                                                  _ptr(self.buf), nbytes.value, C.c_void_p(verdict.data_ptr()), stream))
                self._pending = (verdict, stream, nbytes.value)
                self._hints = None
                return
            flags = (C.c_int32 * 1)(0)
            hints = C.c_int32(0)
            build = lib.m3g_topology_build_canonical if canonical else lib.m3g_topology_build_hints
            _lib.check(build(self.N, self.E, self.T, self.S, _ptr(self.ei), _ptr(self.tei), _ptr(self.batch),
                             _ptr(self.buf), nbytes.value, flags, C.byref(hints) if self.WITH_HINTS else None, _stream()))
        # (the build waits for the stream itself, once, and the flags are final on return: include/m3gnet_hip.h)
        self._raise_on(flags[0])
        # the certificate's word: formed with the build (WITH_HINTS), else asked for before the first m3g_energy_forces call
        self._hints = int(hints.value) if self.WITH_HINTS else None

    @staticmethod
    def _raise_on(flags: int) -> None:
        if flags & 1:
            raise ValueError("edge_index must be sorted by centre atom (row 0), as MaterialGraph builds it")
        if flags & 2:
            raise ValueError("graph index out of range (edge_index / triplet_edge_index / batch)")
        if flags & 4:
            raise ValueError("triplet_edge_index pairs edges that do not share a centre atom")

    def finish(self) -> "_Topology":
        """Complete a build that was only queued (m3g_topology_build_canonical_begin): wait for its stream, take the verdict."""
        if self._pending is not None:
            (verdict, stream, nbytes), self._pending = self._pending, None
            flags = (C.c_int32 * 1)(0)
            hints = C.c_int32(0)
            with _cuda.on_device(self.buf.device):
                _lib.check(_lib.load_library().m3g_topology_build_canonical_end(
                    self.N, self.E, self.T, self.S, _ptr(self.ei), _ptr(self.tei), _ptr(self.batch), _ptr(self.buf), nbytes,
                    C.c_void_p(verdict.data_ptr()), flags, C.byref(hints), stream))
            self._raise_on(flags[0])
            self._hints = int(hints.value)
        return self

    def query_hints(self) -> int:
        """The word m3g_topology_hints returns for this topology (certifies complete triplet lists for the three-body moment
        kernels; a few small kernels and one wait for the stream).  Cached."""
        self.finish()
        if self._hints is None:
            hints = C.c_int32(0)
            with _cuda.on_device(self.buf.device):
                _lib.check(_lib.load_library().m3g_topology_hints(self.N, self.E, self.T, self.S, _ptr(self.buf), C.byref(hints), _stream()))
            self._hints = int(hints.value)
        return self._hints

    def hints_for_call(self) -> int:
        """m3g_io.topo_hints for m3g_energy_forces calls with this topology: asked for before the first call, so that every
        evaluation of a graph runs the same kernels (bit-identical results from the first call on).  The certificate costs a
        topology that is used once about 0.08 ms on the 10k-atom cell -- `Engine.topology_hints = False` turns it off for such
        loops (the list kernels, always valid)."""
        return self.query_hints()

    def status(self) -> int:
        """Sticky error bits the hot call left on this topology buffer (m3g_topology_status; 0 = none)."""
        self.finish()
        st = C.c_int32(0)
        with _cuda.on_device(self.buf.device):
            _lib.check(_lib.load_library().m3g_topology_status(self.N, self.E, self.T, self.S, _ptr(self.buf), C.byref(st), _stream()))
        return int(st.value)

    def n_active(self) -> int:
        """Edges that take part in a triplet (rows of the three-body arrays)."""
        self.finish()
        n = C.c_int64()
        with _cuda.on_device(self.buf.device):
            _lib.check(_lib.load_library().m3g_topology_active_edges(self.N, self.E, self.T, self.S, _ptr(self.buf), C.byref(n), _stream()))
        return int(n.value)

    @staticmethod
    def signature(graph):
        sig = []
        for key in (K.EDGE_INDEX, K.TRIPLET_EDGE_INDEX, K.BATCH):
            t = graph[key]
            sig.append((t.data_ptr(), t._version, tuple(t.shape)))
        sig.append(int(graph[K.LATTICE].size(0)))
        return tuple(sig)

    @classmethod
    def of(cls, graph, finish: bool = True) -> "_Topology":
        """The topology of `graph`, built on first use and cached on the graph.  `finish=False`: a build that was only queued (see
        `__init__`) is returned as it is; the caller calls `finish()` before it hands the buffer to a kernel."""
        sig = cls.signature(graph)
        cached = graph.get("_m3g_topology") if isinstance(graph, dict) else None
        if cached is not None and cached[0] == sig:
            topo = cached[1]
        else:
            topo = cls(graph, sig)
            if isinstance(graph, dict):
                dict.__setitem__(graph, "_m3g_topology", (sig, topo))
        return topo.finish() if finish else topo


# ----------------------------------------------------------------------------------------------
_OUT_OF_RANGE = "graph index out of range (edge_index / triplet_edge_index / batch)"   # (the text `_Topology._raise_on` gives)


def check_index_ranges(n_atoms: int, n_edges: int, n_structs: int, edge_index=None, triplet_edge_index=None, batch=None) -> None:
    """Host-side range check of a graph's index tensors (CPU or GPU tensors; None: not checked), for the modules whose kernels index
    with the caller's own lists instead of a `_Topology` (m3g_three_body, m3g_readout: no range check on the device).  edge_index
    [2, n_edges] must lie in [0, n_atoms), triplet_edge_index [2, T] in [0, n_edges), batch [n_atoms] in [0, n_structs); otherwise
    ValueError with the text of the fused path's refusal -- raised before any kernel of the library is enqueued."""
    for t, bound, shape, name in ((edge_index, n_atoms, (2, n_edges), K.EDGE_INDEX), (triplet_edge_index, n_edges, (2, None), K.TRIPLET_EDGE_INDEX),
                                  (batch, n_structs, (n_atoms,), K.BATCH)):
        if t is None:
            continue
        if t.dim() != len(shape) or any(want is not None and int(have) != int(want) for have, want in zip(t.shape, shape)):
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not match the graph's sizes (expected {shape})")
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.is_complex():
            raise ValueError(f"{name}: an integer tensor is required")
        if t.numel() == 0:
            continue
        lo, hi = torch.aminmax(t)
        if int(lo) < 0 or int(hi) >= bound:
            raise ValueError(_OUT_OF_RANGE)


def _indices_already_checked(graph, n_atoms: int, n_edges: int, n_structs: int) -> bool:
    """True where the graph carries a `_Topology` built from its present index tensors (its build has range-checked all three)."""
    cached = graph.get("_m3g_topology") if isinstance(graph, dict) else None
    if cached is None or any(key not in graph for key in (K.EDGE_INDEX, K.TRIPLET_EDGE_INDEX, K.BATCH, K.LATTICE)):
        return False
    if cached[0] != _Topology.signature(graph):
        return False
    topo = cached[1].finish()
    return (topo.N, topo.E, topo.S) == (n_atoms, n_edges, n_structs)


def _require_rows(t: torch.Tensor, shape, name: str) -> None:
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")


# ----------------------------------------------------------------------------------------------
class ScaleLength(torch.nn.Module):
    """pos, lattice -> scaled_pos, scaled_lattice (reference nn/scale.py:8-29).  In the fused path the
    division happens inside the geometry kernel; standalone it is a device-side elementwise op."""

    def __init__(self, length_scale: float):
        super().__init__()
        self.length_scale = length_scale

    def forward(self, graph):
        _require_cuda(graph[K.POS], K.POS)
        graph[K.SCALED_POS] = graph[K.POS] / self.length_scale
        graph[K.SCALED_LATTICE] = graph[K.LATTICE] / self.length_scale
        return graph


class AtomRef(torch.nn.Module):
    """elemental_energies[atom_types] (reference nn/atom_ref.py:10-29)."""

    def __init__(self, elemental_energies: torch.Tensor, device: torch.device | None = None):
        super().__init__()
        self.elemental_energies = elemental_energies.to(device)

    def forward(self, graph):
        types = graph[K.ATOM_TYPES]
        _require_cuda(types, K.ATOM_TYPES)
        table = self.elemental_energies.to(device=types.device, dtype=torch.float).contiguous()
        out = torch.empty(types.numel(), dtype=torch.float, device=types.device)
        lib = _lib.load_library()
        types = types.contiguous().long()
        _lib.check(lib.m3g_atom_ref(table.numel(), _ptr(table), types.numel(), _ptr(types), _ptr(out), _stream()))
        graph[K.ELEMENTAL_ENERGIES] = out
        return graph


class DistanceAndAngle(torch.nn.Module):
    """edge_distances and clamped cos(theta_jik) from scaled positions (reference nn/invariant.py:8-59)."""

    def forward(self, graph):
        pos, lat = graph[K.SCALED_POS], graph[K.SCALED_LATTICE]
        _require_cuda(pos, K.SCALED_POS)
        topo = _Topology.of(graph)
        pos = pos.contiguous().float()
        lat = lat.contiguous().float()
        shift = graph[K.EDGE_CELL_SHIFT].contiguous().to(torch.int32)
        dist = torch.empty(topo.E, dtype=torch.float, device=pos.device)
        ang = torch.empty(topo.T, dtype=torch.float, device=pos.device)
        scratch = torch.empty(max(topo.E, 1) * 3, dtype=torch.float, device=pos.device)
        lib = _lib.load_library()
        _lib.check(lib.m3g_distance_angle(1.0, topo.N, topo.E, topo.T, topo.S, _ptr(pos), _ptr(lat), _ptr(shift), _ptr(topo.buf),
                                          _ptr(topo.tei), _ptr(scratch), _ptr(dist), _ptr(ang), _stream()))
        graph[K.EDGE_DISTANCES] = dist
        graph[K.TRIPLET_ANGLES] = ang
        return graph


class AtomFeaturizer(torch.nn.Module):
    """One-hot(species) @ W^T, i.e. a row gather of W^T (reference nn/featurizer.py:11-38)."""

    def __init__(self, num_types: int, embedding_dim: int, device: torch.device | None = None):
        super().__init__()
        self._num_types = num_types
        self.linear = torch.nn.Linear(num_types, embedding_dim, bias=False, device=device)

    @property
    def num_types(self) -> int:
        return self._num_types

    def forward(self, graph):
        types = graph[K.ATOM_TYPES]
        _require_cuda(types, K.ATOM_TYPES)
        w = self.linear.weight.detach().to(device=types.device, dtype=torch.float).contiguous()
        types = types.contiguous().long()
        x = torch.empty(types.numel(), w.size(0), dtype=torch.float, device=types.device)
        lib = _lib.load_library()
        _lib.check(lib.m3g_atom_featurizer(self._num_types, w.size(0), _ptr(w), types.numel(), _ptr(types), _ptr(x), _stream()))
        graph[K.NODE_FEATURES] = x
        return graph


class EdgeFeaturizer(torch.nn.Module):
    """Orthogonalised sinc-pair radial basis (reference nn/featurizer.py:41-100)."""

    def __init__(self, degree: int, cutoff: float, device: torch.device | None = None):
        super().__init__()
        self.degree, self.cutoff, self.device = degree, cutoff, device
        idx = torch.arange(degree, device=device)
        # e_m = m^2 (m+2)^2 / (4 (m+1)^4 + 1);  d_0 = 1, d_m = 1 - e_m / d_{m-1}
        self.em = (idx**2) * ((idx + 2) ** 2) / (4 * ((idx + 1) ** 4) + 1)
        dm = torch.ones(degree, device=device)
        for m in range(1, degree):
            dm[m] = 1 - self.em[m] / dm[m - 1]
        self.dm = dm
        coeff = torch.empty(degree)
        for m in range(degree):
            sign = -1 if m % 2 else 1
            coeff[m] = sign * np.sqrt(2) * np.pi / (cutoff**1.5) * (m + 1) * (m + 2) / np.sqrt((m + 1) ** 2 + (m + 2) ** 2)
        self.coeff = coeff.to(device)

    def host_constants(self):
        f = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)  # noqa: E731
        return f(self.em), f(self.dm), f(self.coeff)

    def forward(self, graph):
        dist = graph[K.EDGE_DISTANCES]
        _require_cuda(dist, K.EDGE_DISTANCES)
        dist = dist.contiguous().float()
        out = torch.empty(dist.numel(), self.degree, dtype=torch.float, device=dist.device)
        em, dm, coeff = self.host_constants()
        lib = _lib.load_library()
        _lib.check(lib.m3g_edge_featurizer(self.degree, float(self.cutoff), em.ctypes.data, dm.ctypes.data, coeff.ctypes.data,
                                           dist.numel(), _ptr(dist), _ptr(out), _stream()))
        graph[K.EDGE_WEIGHTS] = out
        return graph


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().float()


def _param_ptr_array(tensors):
    """HOST array of DEVICE pointers (the `host_params` argument of m3g_conv_block / m3g_readout); returns (array, keep-alive)."""
    keep = [_f32(t) for t in tensors]
    arr = (C.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
    return arr, keep


def _linear(x: torch.Tensor, lin: torch.nn.Linear, act: int) -> torch.Tensor:
    """act(x W^T + b) through m3g_linear (act 0 none, 1 SiLU, 2 sigmoid)."""
    _require_cuda(x, "input")
    x2 = _f32(x).reshape(-1, lin.in_features)
    w = _f32(lin.weight).to(x2.device)
    b = _f32(lin.bias).to(x2.device) if lin.bias is not None else None
    y = torch.empty(x2.size(0), lin.out_features, dtype=torch.float, device=x2.device)
    with _cuda.on_device(x2.device):
        _lib.check(_lib.load_library().m3g_linear(x2.size(0), lin.in_features, lin.out_features, _ptr(x2), _ptr(w), _ptr(b), act, _ptr(y), _stream()))
    return y.reshape(*x.shape[:-1], lin.out_features)


class EdgeAdjustor(torch.nn.Module):
    """edge_attr = SiLU(W edge_weights) (reference nn/featurizer.py:103-132)."""

    def __init__(self, degree: int, num_edge_features: int, device: torch.device | None = None):
        super().__init__()
        self.degree, self.num_edge_features = degree, num_edge_features
        self.linear = torch.nn.Linear(degree, num_edge_features, bias=False, device=device)
        self.swish = torch.nn.SiLU()

    def forward(self, graph):
        graph[K.EDGE_ATTR] = _linear(graph[K.EDGE_WEIGHTS], self.linear, act=1)   # SiLU(W edge_weights)
        return graph


class GatedMLP(torch.nn.Module):
    """dense(x) * gate(x) (reference nn/core.py:6-62).  Holds the parameters with the reference's
    Sequential numbering (Linear at even indices, activation at odd)."""

    def __init__(self, in_features: int, dimensions: list[int], is_output: bool = False, use_bias: bool = True,
                 device: torch.device | None = None):
        super().__init__()
        self.in_features, self.dimensions, self.is_output, self.use_bias = in_features, dimensions, is_output, use_bias
        self.dense, self.gate = torch.nn.Sequential(), torch.nn.Sequential()
        widths = [in_features] + list(dimensions)
        last = len(dimensions) - 1
        for i in range(len(dimensions)):
            self.dense.append(torch.nn.Linear(widths[i], widths[i + 1], bias=use_bias, device=device))
            if not (is_output and i == last):
                self.dense.append(torch.nn.SiLU())
            self.gate.append(torch.nn.Linear(widths[i], widths[i + 1], bias=use_bias, device=device))
            self.gate.append(torch.nn.Sigmoid() if i == last else torch.nn.SiLU())

    @staticmethod
    def _branch(seq: torch.nn.Sequential, x: torch.Tensor) -> torch.Tensor:
        mods = list(seq)
        i = 0
        while i < len(mods):
            lin = mods[i]
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            act = 1 if isinstance(nxt, torch.nn.SiLU) else 2 if isinstance(nxt, torch.nn.Sigmoid) else 0
            x = _linear(x, lin, act)
            i += 2 if act else 1
        return x

    def forward(self, x):
        """dense(x) * gate(x) for any layer widths (m3g_linear per layer, m3g_multiply for the product)."""
        d, g = self._branch(self.dense, x), self._branch(self.gate, x)
        out = torch.empty_like(d)
        with _cuda.on_device(d.device):
            _lib.check(_lib.load_library().m3g_multiply(d.numel(), _ptr(d), _ptr(g), _ptr(out), _stream()))
        return out


class NormalizedSphericalBessel(torch.nn.Module):
    """chi_ln(r) = j_l(z_ln r / rc) / factors[l, n] (reference nn/interaction.py:226-281).

    `factors` reproduces the reference construction, INCLUDING its evaluation of j_{l+1} at the roots
    of j_{l+1} itself (SURVEY finding 1): it is a captured constant of rounding-noise size, not the
    documented normalisation.  It is a plain attribute; assign another tensor to change it (see
    `documented_factors`)."""

    def __init__(self, cutoff: float, l_max: int, n_max: int, device: torch.device | None = None):
        super().__init__()
        self.cutoff, self.l_max, self.n_max, self.device = cutoff, l_max, n_max, device
        self.spherical_bessel_zeros = torch.tensor(SPHERICAL_BESSEL_ZEROS, device=device)
        if self.spherical_bessel_zeros.size(0) < l_max + 1:
            raise ValueError("Too large l_max is specified.")
        if self.spherical_bessel_zeros.size(1) < n_max:
            raise ValueError("Too large n_max is specified.")
        scale = math.sqrt(2 / (cutoff**3))
        rows = [scale / torch.abs(spherical_bessel(self.spherical_bessel_zeros[l + 1, :n_max], l + 1)) for l in range(l_max)]
        self.factors = torch.stack(rows)

    def documented_factors(self) -> torch.Tensor:
        """`factors` realising sqrt(2/rc^3) j_l(z_ln r/rc) / |j_{l+1}(z_ln)| (reference docs/architecture.md:127-132)."""
        z = torch.tensor(SPHERICAL_BESSEL_ZEROS, dtype=torch.float64)
        scale = math.sqrt(2 / (self.cutoff**3))
        rows = [scale / torch.abs(spherical_bessel(z[l, : self.n_max], l + 1)) for l in range(self.l_max)]
        return (1.0 / torch.stack(rows)).to(torch.float)

    def _host_tables(self):
        z = np.ascontiguousarray(self.spherical_bessel_zeros[: self.l_max, : self.n_max].detach().cpu().numpy(), dtype=np.float32)
        f = np.ascontiguousarray(self.factors.detach().cpu().numpy(), dtype=np.float32)
        return z, f

    def forward(self, rs):
        """chi [l_max, n_max, len(rs)] (reference nn/interaction.py:268-281)."""
        _require_cuda(rs, "rs")
        r = _f32(rs).reshape(-1)
        z, f = self._host_tables()
        out = torch.empty(self.l_max, self.n_max, r.numel(), dtype=torch.float, device=r.device)
        with _cuda.on_device(r.device):
            _lib.check(_lib.load_library().m3g_bessel_basis(self.l_max, self.n_max, float(self.cutoff), z.ctypes.data, f.ctypes.data, r.numel(),
                                                             _ptr(r), _ptr(out), _stream()))
        return out


class ThreeBodyInteration(torch.nn.Module):
    """Three-body edge update (reference nn/interaction.py:138-223; class name spelled as there)."""

    def __init__(self, cutoff: float, threebody_cutoff: float, l_max: int, n_max: int, num_node_features: int,
                 num_edge_features: int, device: torch.device | None = None):
        super().__init__()
        self.cutoff, self.threebody_cutoff = cutoff, threebody_cutoff
        self.l_max, self.n_max, self.degree = l_max, n_max, l_max * n_max
        self.num_node_features, self.num_edge_features, self.device = num_node_features, num_edge_features, device
        self.nsb = NormalizedSphericalBessel(cutoff=cutoff, l_max=l_max, n_max=n_max, device=device)
        self.linear_sigmoid1 = torch.nn.Linear(num_node_features, self.degree, device=device)
        self.gated_mlp = GatedMLP(self.degree, [num_edge_features], use_bias=False, device=device)

    def forward(self, graph):
        """edge_attr += GatedMLP(three-body aggregate) from the graph's edge_distances / triplet_angles / x (m3g_three_body)."""
        x, e = graph[K.NODE_FEATURES], graph[K.EDGE_ATTR]
        _require_cuda(x, K.NODE_FEATURES)
        dev = x.device
        x, e_new = _f32(x), _f32(e).clone()
        ei, tei = graph[K.EDGE_INDEX], graph[K.TRIPLET_EDGE_INDEX]
        d, ang = _f32(graph[K.EDGE_DISTANCES]), _f32(graph[K.TRIPLET_ANGLES])
        if x.dim() != 2 or ei.dim() != 2 or tei.dim() != 2:
            raise ValueError("ThreeBodyInteration.forward: x [N,D], edge_index [2,E] and triplet_edge_index [2,T] are required")
        N, E, T, D, Cc = x.size(0), ei.size(1), tei.size(1), x.size(1), self.degree
        if D != self.num_node_features or self.num_edge_features != D:
            raise ValueError("ThreeBodyInteration.forward: m3g_three_body updates edge_attr of the node features' width "
                             f"(num_node_features = num_edge_features = x.size(1)); got {self.num_node_features}, {self.num_edge_features}, {D}")
        _require_rows(e_new, (E, D), K.EDGE_ATTR)
        _require_rows(d, (E,), K.EDGE_DISTANCES)
        _require_rows(ang, (T,), K.TRIPLET_ANGLES)
        # the kernel indexes dist[e], edge_index[1][e], v[k] and its aggregate with these lists as they are: checked here, on the host
        if not _indices_already_checked(graph, N, E, int(graph[K.LATTICE].size(0)) if K.LATTICE in graph else -1):
            check_index_ranges(N, E, 0, edge_index=ei, triplet_edge_index=tei)
        ei, tei = ei.contiguous().long(), tei.contiguous().long()
        z, f = self.nsb._host_tables()
        scratch = torch.empty(N * Cc + E * Cc + 2 * E * D + 16, dtype=torch.float, device=dev)
        mid = torch.empty(E, Cc, dtype=torch.float, device=dev)
        ws, bs = _f32(self.linear_sigmoid1.weight).to(dev), _f32(self.linear_sigmoid1.bias).to(dev)
        wd, wg = _f32(self.gated_mlp.dense[0].weight).to(dev), _f32(self.gated_mlp.gate[0].weight).to(dev)
        with _cuda.on_device(dev):
            _lib.check(_lib.load_library().m3g_three_body(
                self.l_max, self.n_max, D, float(self.cutoff), float(self.threebody_cutoff), z.ctypes.data, f.ctypes.data, N, E, T, _ptr(ei),
                _ptr(tei), _ptr(d), _ptr(ang), _ptr(x), _ptr(ws), _ptr(bs), _ptr(wd), _ptr(wg), _ptr(scratch), _ptr(e_new), _ptr(mid), _stream()))
        graph[K.EDGE_ATTR] = e_new
        graph[K.MID_EDGE_FEATURES] = mid
        return graph


class M3GNetConv(torch.nn.Module):
    """Gated edge update then gated node update with centre-atom aggregation (reference nn/conv.py:12-97)."""

    def __init__(self, degree: int, num_node_features: int, num_edge_features: int, device: torch.device | None = None):
        super().__init__()
        self.degree, self.num_node_features, self.num_edge_features = degree, num_node_features, num_edge_features
        self.num_concat_features = 2 * num_node_features + num_edge_features
        self.concat_edge_update = GatedMLP(self.num_concat_features, [num_edge_features, num_edge_features], device=device)
        self.edge_linear = torch.nn.Linear(degree, num_edge_features, bias=False, device=device)
        self.concat_node_update = GatedMLP(self.num_concat_features, [num_edge_features, num_node_features], device=device)
        self.node_linear = torch.nn.Linear(degree, num_node_features, bias=False, device=device)

    def forward(self, graph):
        """Gated edge update, then gated node update aggregated onto the centre atoms (m3g_conv_block)."""
        x, e = graph[K.NODE_FEATURES], graph[K.EDGE_ATTR]
        _require_cuda(x, K.NODE_FEATURES)
        dev = x.device
        topo = _Topology.of(graph)
        x_new, e_new, h = _f32(x).clone(), _f32(e).clone(), _f32(graph[K.EDGE_WEIGHTS])
        D = x_new.size(1)
        tensors = []
        for mlp, lin in ((self.concat_edge_update, self.edge_linear), (self.concat_node_update, self.node_linear)):
            tensors += [mlp.dense[0].weight, mlp.gate[0].weight, mlp.dense[0].bias, mlp.gate[0].bias,
                        mlp.dense[2].weight, mlp.gate[2].weight, mlp.dense[2].bias, mlp.gate[2].bias, lin.weight]
        params, keep = _param_ptr_array([t.to(dev) for t in tensors])
        lib = _lib.load_library()
        nbytes = C.c_size_t()
        _lib.check(lib.m3g_conv_block_scratch_bytes(D, topo.E, C.byref(nbytes)))
        scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        with _cuda.on_device(dev):
            _lib.check(lib.m3g_conv_block(D, self.degree, topo.N, topo.E, topo.T, topo.S, _ptr(topo.buf), params, _ptr(h), _ptr(x_new), _ptr(e_new),
                                          _ptr(scratch), nbytes.value, _stream()))
            torch.cuda.current_stream().synchronize()   # `keep` and `scratch` are released when this returns
        graph[K.NODE_FEATURES], graph[K.EDGE_ATTR] = x_new, e_new
        return graph


class AtomWiseReadout(torch.nn.Module):
    """Per-atom gated MLP to a scalar, summed per structure (reference nn/readout.py:12-58)."""

    def __init__(self, in_features: int, num_layers: int, scale: float, device: torch.device | None = None):
        super().__init__()
        self.in_features, self.num_layers, self.scale = in_features, num_layers, scale
        self.gated = GatedMLP(in_features, [in_features] * (num_layers - 1) + [1], is_output=True, device=device)

    def forward(self, graph):
        """Per-atom gated MLP, elemental reference added, per-structure sums (m3g_readout)."""
        x = graph[K.NODE_FEATURES]
        _require_cuda(x, K.NODE_FEATURES)
        if self.num_layers != 3:
            raise ValueError("AtomWiseReadout.forward: m3g_readout implements the readout of build_model (num_layers = 3, "
                             f"reference model/build.py:69-76); got num_layers = {self.num_layers}")
        dev = x.device
        x = _f32(x)
        N, D = x.shape
        batch = graph[K.BATCH]
        S = int(graph[K.LATTICE].size(0))
        elem = _f32(graph[K.ELEMENTAL_ENERGIES])
        if D != self.in_features:
            raise ValueError(f"AtomWiseReadout.forward: x has {D} features, the module {self.in_features}")
        _require_rows(elem, (N,), K.ELEMENTAL_ENERGIES)
        # the kernel adds into scaled_total[batch[a]] as it is: checked here, on the host
        if not _indices_already_checked(graph, N, int(graph[K.EDGE_INDEX].size(1)) if K.EDGE_INDEX in graph else -1, S):
            check_index_ranges(N, 0, S, batch=batch)
        batch = batch.contiguous().long()
        tensors = []
        for seq in (self.gated.dense, self.gated.gate):
            for i in (0, 2, 4):
                tensors += [seq[i].weight, seq[i].bias]
        params, keep = _param_ptr_array([t.to(dev) for t in tensors])
        ea = torch.empty(N, dtype=torch.float, device=dev)
        st, tot = torch.empty(S, dtype=torch.float, device=dev), torch.empty(S, dtype=torch.float, device=dev)
        scratch = torch.empty(4 * N * D + 2 * N + 16, dtype=torch.float, device=dev)   # (+16: never an empty buffer)
        with _cuda.on_device(dev):
            _lib.check(_lib.load_library().m3g_readout(D, N, S, params, float(self.scale), _ptr(x), _ptr(elem), _ptr(batch), _ptr(ea), _ptr(st),
                                                       _ptr(tot), _ptr(scratch), _stream()))
            torch.cuda.current_stream().synchronize()
        graph[K.SCALED_ATOMIC_ENERGIES], graph[K.SCALED_TOTAL_ENERGY], graph[K.TOTAL_ENERGY] = ea, st, tot
        return graph


class Gradient(torch.nn.Module):
    """Energies + forces + virial stresses (reference nn/gradient.py:10-64) as one fused engine call.

    The wrapped `model` must be the Sequential laid out by `build_model` (model/build.py:37-76);
    forces come from the engine's analytic reverse pass, not from autograd."""

    def __init__(self, model: torch.nn.Module, pair_virial: bool = False, legendre_backward: str = "exact"):
        """`pair_virial=False` reproduces the reference's stress formula sum_a pos_a (x) F_a / V (nn/gradient.py:39-62,
        absolute positions -- not invariant under a lattice translation of an atom); `pair_virial=True` returns the
        strain derivative -(1/V) sum_e r_e (x) dE/dr_e over the pair vectors (docs/gradient.md:47-84).

        `legendre_backward="exact"`: forces are the gradient of the energy.  `"reference"`: d P_l / d cos(theta) is what the
        reference's LegendreCosPolynomial.backward returns (nn/interaction.py:373-382, inexact for l >= 2), so forces and
        stresses reproduce the reference's own numbers (engine option "legendre_backward"; the three-body list kernels run)."""
        super().__init__()
        if legendre_backward not in ("exact", "reference"):
            raise ValueError('legendre_backward: "exact" or "reference"')
        self.model = model
        self.legendre_backward = legendre_backward
        self.pair_virial = bool(pair_virial)
        self._engine = None

    @property
    def engine(self):
        if self._engine is None:
            from ..engine import Engine

            self._engine = Engine(self.model)
            self._engine.set_option("stress_mode", 1 if self.pair_virial else 0)
            self._engine.set_option("legendre_backward", 1 if self.legendre_backward == "reference" else 0)
        return self._engine

    def forward(self, graph, forces: bool = True, extras: bool = True):
        return self.engine.run(graph, want_forces=forces, extras=extras)
